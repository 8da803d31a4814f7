// Optimized tetrahedron method (gfx950 only): what the two producers of node weights of the optimized rule share -- the real
// weights w_b(k; E) of kernels_ltm_opt_nodew.hip and the complex weights W_b(k; z) of kernels_ltm_green_opt_nodew.hip.  Each
// file has its own corner-weight kernel (A); the arguments, the sort step that carries a corner's path position, the select
// tables of a path, the gather kernel (B: it sums any NE real sets of corner weights in one fixed order) and the slab planner of
// the workspace are the same and stand here.  kernels_ltm_opt_nodew.hip has the definition, the layout of the workspace and
// the reasoning about slabs.
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

// index i - o of a periodic axis of npt >= 1 points, o in -1 .. 2
__device__ __forceinline__ int optw_wrap_back(int i, int o, int npt) {
    int j = i - o;
    j += j < 0 ? npt : 0;
    j += j < 0 ? npt : 0;  // npt = 1: i - 2 is two periods away
    j -= j >= npt ? npt : 0;
    return j;
}

// The three select tables of a path, as in ltm_opt_kernel: what the step o - 1 along the path's first, second and third axis
// adds to the column and to the line.  j1, j2: wrapped indices of the axes 1, 2; j3: of axis 3, times npt.
#define OPTW_TABLES(t, j1, j2, j3)                                                  \
    const int X = (t) >> 1, Y = (X + 1 + ((t) & 1)) % 3, Z = 3 - X - Y;             \
    int col[3][4], line[3][4];                                                      \
    _Pragma("unroll") for (int o = 0; o < 4; ++o) {                                 \
        col[0][o] = X == 0 ? j1[o] : 0;                                             \
        col[1][o] = Y == 0 ? j1[o] : 0;                                             \
        col[2][o] = Z == 0 ? j1[o] : 0;                                             \
        line[0][o] = X == 1 ? j2[o] : (X == 2 ? j3[o] : 0);                         \
        line[1][o] = Y == 1 ? j2[o] : (Y == 2 ? j3[o] : 0);                         \
        line[2][o] = Z == 1 ? j2[o] : (Z == 2 ? j3[o] : 0);                         \
    }
#define OPTW_COL(j) (col[0][OPT_PT[j][0] + 1] + col[1][OPT_PT[j][1] + 1] + col[2][OPT_PT[j][2] + 1])
#define OPTW_LINE(j) (line[0][OPT_PT[j][0] + 1] + line[1][OPT_PT[j][1] + 1] + line[2][OPT_PT[j][2] + 1])

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
        OPTW_TABLES(tt, j1, j2, j3)
        const double* __restrict__ const Ct = Cb + (int64_t)(tt * 4) * a.wsplane;
#pragma unroll
        for (int j = 0; j < OPT_NPT; ++j) {
            const double* __restrict__ const Cj = Ct + ((int64_t)OPTW_LINE(j) * npt + OPTW_COL(j));
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

}  // namespace

}  // namespace abz
