// Optimized tetrahedron method (gfx950 only): what the two producers of node weights of the optimized rule share -- the real
// weights w_b(k; E) of kernels_ltm_opt_nodew.hip and the complex weights W_b(k; z) of kernels_ltm_green_opt_nodew.hip.  Each
// file has its own corner-weight kernel (A) and its own grouping of energies or values of z; the arguments, the prologue of a
// corner-weight kernel, the sort that carries a corner's path position and the select back to path order, the gather kernel (B:
// it sums any NE real sets of corner weights in one fixed order), the slab planner of the workspace and the slab loop of the
// host are the same and stand here.  The stencil addressing is OptPath of ltm_opt_device.h.  kernels_ltm_opt_nodew.hip has the
// definition, the layout of the workspace and the reasoning about slabs.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abz_internal.h"
#include "ltm_opt_device.h"

namespace abz {

namespace {

struct OptWArgs {
    PlaneView E, W;  // eigenvalue planes; the weight block (nE n planes per tile, pitch = row)
    double* C;       // workspace [n][NE][24][nplanes npt^2]
    int64_t wsplane; // cells of the workspace: nplanes npt^2
    int npt;
    int n;
    int nplanes;     // cell planes in the workspace
    int cell0;       // grid plane of the workspace's plane 0, inside 0 .. npt-1
    int node0;       // first node plane of the slab (B)
    int nnode;       // node planes of the slab (B)
    int wrap3;       // B: the workspace holds the whole grid, plane = grid plane mod npt (else plane = grid plane - (node0 - 2))
    int plane0;      // first weight plane of this launch: (its first energy) * n
    double weight;   // 1 / (6 npt^3)
    double Es[4];    // the launch's energies (NE of them)
};

// compare-exchange of two corners: the energies, and each corner's position in the path with them
__device__ __forceinline__ void optw_cx(double& ea, double& eb, int& pa, int& pb) {
    const bool sw = eb < ea;
    const double lo = sw ? eb : ea, hi = sw ? ea : eb;
    const int x = sw ? pb : pa, y = sw ? pa : pb;
    ea = lo;
    eb = hi;
    pa = x;
    pb = y;
}

// the four effective corner energies of a simplex ascending, e1 <= .. <= e4, and the position in the path of each: p1 .. p4
struct OptWSorted {
    double e1, e2, e3, e4;
    int p1, p2, p3, p4;
};
__device__ __forceinline__ OptWSorted optw_sort(const double (&e)[4]) {
    OptWSorted s = {e[0], e[1], e[2], e[3], 0, 1, 2, 3};
    optw_cx(s.e1, s.e2, s.p1, s.p2);
    optw_cx(s.e3, s.e4, s.p3, s.p4);
    optw_cx(s.e1, s.e3, s.p1, s.p3);
    optw_cx(s.e2, s.e4, s.p2, s.p4);
    optw_cx(s.e2, s.e3, s.p2, s.p3);
    return s;
}
// back to path order: corner m of the path is the sorted corner whose position is m
__device__ __forceinline__ double optw_of_path(const OptWSorted& s, int m, double w1, double w2, double w3, double w4) {
    return s.p1 == m ? w1 : (s.p2 == m ? w2 : (s.p3 == m ? w3 : w4));
}

// index i - o of a periodic axis of npt >= 1 points, o in -1 .. 2
__device__ __forceinline__ int optw_wrap_back(int i, int o, int npt) {
    int j = i - o;
    j += j < 0 ? npt : 0;
    j += j < 0 ? npt : 0;  // npt = 1: i - 2 is two periods away
    j -= j >= npt ? npt : 0;
    return j;
}

// What a thread of a corner-weight kernel (A) starts from: cell kk < a.wsplane of the workspace (column i1 of line i2 of its
// plane q, which is grid plane cell0 + q wrapped) -> the index tables of its stencil on the grid, the eigenvalue planes of band
// blockIdx.y (a 32-bit line stride: the host checks that it fits) and where its corner weights go: plane [t 4 + m] of set s of
// this band is out[(s 24 + t 4 + m) wsplane], `sets` sets per band.  The arguments come by value: by reference
// ltm_green_opt_cornerw_kernel<1> compiles to 34 SGPR spills instead of 26 (profiles/ltm_opt_shared_stencil_isa_vs_parent.txt).
struct OptWCell {
    int j1[4], j2[4], j3[4];
    const double* Eb;
    int tileE;
    double* out;
};
__device__ __forceinline__ OptWCell optw_cell(OptWArgs a, int64_t kk, int sets) {
    const LtmCell cell = ltm_cell<3>(kk, a.npt);
    int i3 = a.cell0 + cell.i3;
    i3 -= i3 >= a.npt ? a.npt : 0;
    OptWCell c;
    opt_tables(cell.i1, cell.i2, i3, a.npt, c.j1, c.j2, c.j3);
    c.Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    c.tileE = (int)a.E.tile;
    c.out = a.C + (int64_t)blockIdx.y * sets * 24 * a.wsplane + kk;
    return c;
}

// ---------------------------------------------------------------------------------------------------------------------
// B: the node's weight, gathered from the corner weights of the simplices whose stencil holds it
// ---------------------------------------------------------------------------------------------------------------------
// Thread t of the launch is column t % row of line t / row of the slab's node planes, as in ltm_nodew_kernel.
template <int NE>
__global__ __launch_bounds__(256) void ltm_opt_nodew_gather_kernel(OptWArgs a) {
    const int row = a.W.row, npt = a.npt;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)a.nnode * npt * row) return;
    const int lline = (int)(t <= 0xffffffffll ? (int64_t)((uint32_t)t / (uint32_t)row) : t / row);  // line inside the slab (below npt^2)
    const int i1 = (int)(t - (int64_t)lline * row);
    const int l3 = (int)((uint32_t)lline / (uint32_t)npt);
    const int i2 = lline - l3 * npt, i3 = a.node0 + l3;
    const int64_t gline = (int64_t)i3 * npt + i2;
    double* __restrict__ const out = a.W.base + gline * a.W.tile + (int64_t)(a.plane0 + (int)blockIdx.y) * a.W.pitch + i1;
    const int64_t wstep = (int64_t)a.n * a.W.pitch;  // from an energy's plane of this band to the next energy's
    if (i1 >= npt) {
#pragma unroll
        for (int i = 0; i < NE; ++i) out[i * wstep] = 0.0;
        return;
    }
    // the cell k - o of every axis, o = -1 .. 2: a column, a line of the workspace's plane, a plane of the workspace (times npt)
    int j1[4], j2[4], j3[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        j1[o] = optw_wrap_back(i1, o - 1, npt);
        j2[o] = optw_wrap_back(i2, o - 1, npt);
        j3[o] = (a.wrap3 ? optw_wrap_back(i3, o - 1, npt) : l3 + 2 - (o - 1)) * npt;
    }
    const double* __restrict__ const Cb = a.C + (int64_t)blockIdx.y * NE * 24 * a.wsplane;
    double acc[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) acc[i] = 0.0;
#pragma unroll 1
    for (int tt = 0; tt < 6; ++tt) {
        const OptPath path(tt, j1, j2, j3);
        const double* __restrict__ const Ct = Cb + (int64_t)(tt * 4) * a.wsplane;
#pragma unroll
        for (int j = 0; j < OPT_NPT; ++j) {
            const double* __restrict__ const Cj = Ct + ((int64_t)path.line_of(j) * npt + path.col_of(j));
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                if (OPT_K[m][j] == 0) continue;
#pragma unroll
                for (int i = 0; i < NE; ++i) acc[i] = fma((double)OPT_K[m][j] / 1260.0, Cj[(int64_t)(i * 24 + m) * a.wsplane], acc[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) out[i * wstep] = a.weight * acc[i];
}

// The slab height of a group of `sets` real weight sets under a cap of `mb` MB: S + 3 planes of 24 n sets doubles per cell within
// the cap, S >= 1.  One slab of npt wrapped planes where those S + 3 planes hold the whole grid.
inline int optw_slab(int npt, int n, int sets, int64_t mb) {
    const int64_t plane_bytes = (int64_t)sizeof(double) * 24 * n * sets * ((int64_t)npt * npt);
    const int64_t fit = (mb << 20) / plane_bytes;
    return (int)std::min<int64_t>(npt, std::max<int64_t>(1, fit - 3));
}
// cell planes in the workspace of a slab of S node planes
inline int optw_planes_of(int npt, int S) { return S + 3 >= npt ? npt : S + 3; }
// the cap of the workspace, MB
inline int64_t optw_cap_mb() { return abz_switch(SW_LTM_OPTW_CHUNK_MB) > 0 ? abz_switch(SW_LTM_OPTW_CHUNK_MB) : 256; }
// bytes of workspace that a group of `sets` real weight sets asks for
inline size_t optw_need(int npt, int n, int sets) {
    return sizeof(double) * 24 * (size_t)n * (size_t)sets * (size_t)optw_planes_of(npt, optw_slab(npt, n, sets, optw_cap_mb())) * (size_t)npt * (size_t)npt;
}

// THE slab loop: one group of `sets` real weight sets, slab after slab -- the corner weights of a slab's cells into the workspace
// a.C (at least optw_need(npt, n, sets) bytes), then the gather into the slab's node planes of a.W.  Of `a` everything but the
// slab's own fields is set by the caller: E, W, C, npt, n, weight, and of the group Es and plane0.  Launches only.
using OptWFn = void (*)(OptWArgs);
inline int optw_run_group(abz_ctx* ctx, OptWArgs& a, int sets, OptWFn corner, OptWFn gather) {
    const int npt = a.npt;
    const int64_t cells = (int64_t)npt * npt;  // of a plane
    const int S = optw_slab(npt, a.n, sets, optw_cap_mb());
    const bool whole = S + 3 >= npt;
    for (int s0 = 0; s0 < npt; s0 += whole ? npt : S) {
        a.node0 = s0;
        a.nnode = whole ? npt : std::min(S, npt - s0);
        a.nplanes = whole ? npt : a.nnode + 3;
        a.wrap3 = whole;
        a.cell0 = whole ? 0 : (s0 + npt - 2) % npt;  // (S + 3 < npt here: npt >= 5)
        a.wsplane = (int64_t)a.nplanes * cells;
        launch(ctx, corner, dim3((unsigned)cdiv64(a.wsplane, 256), (unsigned)a.n), dim3(256), 0, a);
        ABZ_HIP(hipGetLastError());
        launch(ctx, gather, dim3((unsigned)cdiv64((int64_t)a.nnode * npt * a.W.row, 256), (unsigned)a.n), dim3(256), 0, a);
        ABZ_HIP(hipGetLastError());
    }
    return ABZ_OK;
}

}  // namespace

}  // namespace abz
