// Optimized tetrahedron method (gfx950 only): the complex integration weights W_b(k; z) of the Green's function per grid point
// and band, of the rule of kernels_ltm_green_opt.hip, d = 3, written into a block laid out like that of
// kernels_ltm_green_nodew.hip (2 nz real weight sets: plane (2 i + part) n + b is Re / Im of band b at z_i).
//
//  * Definition.  For every Kuhn simplex T (path t, cell i) and band b: e'_m = sum_j P[m][j] e_b(p_j) (ltm_opt_device.h), and
//    W'_m(T; z) = J[sort(e'_1 .. e'_4), e'_m](z) / 4, m = 1..4, are the corner weights of green_weights<4> (ltm_green_device.h, which
//    returns 4 W') brought back to path order.  An element takes the same projection, so the corner weights are scattered with P
//    transposed onto the 20 stencil points, exactly as the real weights of kernels_ltm_opt_nodew.hip are:
//        W_b(k; z) = 1 / (6 npt^3) sum_t sum_{j = 1..20} sum_{m = 1..4} P[m][j] W'_m(T = (t, cell k - off_{t,j}); z),
//    every index wrapped mod npt.  sum_k sum_b W A is then the G_A(z) of abz_rule_ltm_green_optimized for ANY A, sum W = tr G(z) and
//    sum W e = z tr G - n.  Im z < 0: computed at conj(z) and conjugated where the corner weights are stored: the conjugate of
//    the weights at conj(z) to the bit.
//  * Two kernels per group of NZ = 1 or 2 values of z (by value), no atomics anywhere:
//    A'. ltm_green_opt_cornerw_kernel<NZ>: the cell walk and the table and select addressing of ltm_opt_cornerw_kernel (one cell
//       per thread, blockIdx.y the band, the six simplices under unroll 1, nothing indexed at run time, a 32-bit line stride
//       that the host checks).  Per simplex 20 loads, opt_project, the five-step compare-exchange sort that carries each corner's
//       path position, the four corner logs (taken after the sort), green_weights<4> per z, and 8 NZ stores in path order into the
//       workspace [band][set][t 4 + m][cell] as 2 NZ real sets: set 2 iz = Re, set 2 iz + 1 = Im with the sign of Im z applied.
//       Every simplex stores: the workspace needs no clearing.
//    B. ltm_opt_nodew_gather_kernel<2 NZ> (ltm_opt_nodew_device.h), the gather of the real weights as it is: it sums the 432 terms
//       of a node per set in one fixed order (t, j, m) and writes plane (plane0 / n + set) n + b, which is the layout of the complex
//       block.  The host's scale is 1 / (24 npt^3): of a simplex, and of its corner weights the 1 / 4.
//  * Workspace and slabs: scratch[1] under ABZ_LTM_OPTW_CHUNK_MB and the slab planner of the real weights (optw_slab) for 2 NZ
//    sets.  A node's terms and their order do not depend on the slab height: the block has the same bits for every cap.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_green_device.h"
#include "ltm_opt_device.h"
#include "ltm_opt_nodew_device.h"

namespace abz {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// A': complex corner weights of every simplex of the workspace's cells.  a.Es holds the launch's z as (re, im) pairs.
// ---------------------------------------------------------------------------------------------------------------------
template <int NZ>
__global__ __launch_bounds__(256) void ltm_green_opt_cornerw_kernel(OptWArgs a) {
    const int64_t kk = (int64_t)blockIdx.x * 256 + threadIdx.x;  // cell of the workspace: column i1 of line i2 of its plane q
    if (kk >= a.wsplane) return;
    const int npt = a.npt;
    const LtmCell cell = ltm_cell<3>(kk, npt);
    int i3 = a.cell0 + cell.i3;  // the grid plane of the workspace's plane
    i3 -= i3 >= npt ? npt : 0;
    const double* __restrict__ const Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    const int tileE = (int)a.E.tile;  // (the host checks that it fits)
    int j1[4], j2[4], j3[4];
#pragma unroll
    for (int o = 0; o < 4; ++o) {
        j1[o] = opt_wrap(cell.i1, o - 1, npt);
        j2[o] = opt_wrap(cell.i2, o - 1, npt);
        j3[o] = opt_wrap(i3, o - 1, npt) * npt;
    }
    double zr[NZ], zi[NZ];
    bool neg[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        zr[i] = a.Es[2 * i];
        zi[i] = fabs(a.Es[2 * i + 1]);
        neg[i] = a.Es[2 * i + 1] < 0.0;
    }
    // plane [t 4 + m] of set s of this band: out[(s 24 + t 4 + m) wsplane]
    double* __restrict__ const out = a.C + (int64_t)blockIdx.y * (2 * NZ) * 24 * a.wsplane + kk;
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        OPTW_TABLES(t, j1, j2, j3)
        double x[OPT_NPT], e[4];
#pragma unroll
        for (int j = 0; j < OPT_NPT; ++j) x[j] = Eb[(int64_t)OPTW_LINE(j) * tileE + OPTW_COL(j)];
        opt_project(x, e);
        double e1 = e[0], e2 = e[1], e3 = e[2], e4 = e[3];
        int p1 = 0, p2 = 1, p3 = 2, p4 = 3;
        optw_cx(e1, e2, p1, p2);
        optw_cx(e3, e4, p3, p4);
        optw_cx(e1, e3, p1, p3);
        optw_cx(e2, e4, p2, p4);
        optw_cx(e2, e3, p2, p3);
        double* __restrict__ const ot = out + (int64_t)(t * 4) * a.wsplane;
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            const double u1 = zr[i] - e1, u2 = zr[i] - e2, u3 = zr[i] - e3, u4 = zr[i] - e4, y = zi[i];
            const GreenCorner g[4] = {{e1, 0.5 * log(u1 * u1 + y * y), atan2(y, u1)},
                                      {e2, 0.5 * log(u2 * u2 + y * y), atan2(y, u2)},
                                      {e3, 0.5 * log(u3 * u3 + y * y), atan2(y, u3)},
                                      {e4, 0.5 * log(u4 * u4 + y * y), atan2(y, u4)}};
            Cx W[4];
            green_weights<4>(g, zr[i], y, W);
            // back to path order: corner m of the path is the sorted corner whose position is m
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const double re = p1 == m ? W[0].re : (p2 == m ? W[1].re : (p3 == m ? W[2].re : W[3].re));
                const double im = p1 == m ? W[0].im : (p2 == m ? W[1].im : (p3 == m ? W[2].im : W[3].im));
                ot[(int64_t)((2 * i) * 24 + m) * a.wsplane] = re;
                ot[(int64_t)((2 * i + 1) * 24 + m) * a.wsplane] = neg[i] ? -im : im;
            }
        }
    }
}

#undef OPTW_TABLES
#undef OPTW_COL
#undef OPTW_LINE

// Values of z per group where at least that many remain.  A' is the expensive kernel and the slab overlap (S + 3) / S multiplies
// it: a pair takes 4 sets and gets shorter slabs under the cap than a single value's 2 sets.  Measured at SVO 150^3 under the default
// cap: 39.6 ms per z alone, 47.7 ms in pairs; where one slab holds the grid the pair is 1.47 times faster.
#ifndef ABZ_LTM_GREEN_OPTW_NZ
#define ABZ_LTM_GREEN_OPTW_NZ 1
#endif
constexpr int green_opt_nodew_nz() { return ABZ_LTM_GREEN_OPTW_NZ; }
static_assert(green_opt_nodew_nz() == 1 || green_opt_nodew_nz() == 2, "a group is one value of z or a pair");

using OptWFn = void (*)(OptWArgs);
// the pair's kernels exist only in a build that launches them
template <int NZ>
constexpr OptWFn green_optw_pair_corner() {
    if constexpr (NZ == 2) return ltm_green_opt_cornerw_kernel<2>;
    else return nullptr;
}
template <int NZ>
constexpr OptWFn green_optw_pair_gather() {
    if constexpr (NZ == 2) return ltm_opt_nodew_gather_kernel<4>;
    else return nullptr;
}
// [NZ == 2]
constexpr OptWFn GREEN_OPTW_CORNER[2] = {ltm_green_opt_cornerw_kernel<1>, green_optw_pair_corner<green_opt_nodew_nz()>()};
constexpr OptWFn GREEN_OPTW_GATHER[2] = {ltm_opt_nodew_gather_kernel<2>, green_optw_pair_gather<green_opt_nodew_nz()>()};

}  // namespace

// The block W (2 nz n planes, tiled like the eigenvalue planes E with pitch = row, padding columns included) <- W_b(k; z_i) of the
// optimized rule, z_host [nz][2] with Im z != 0.  Launches only; groups of green_opt_nodew_nz() values, then single ones; per group
// the slabs one after the other.
int launch_ltm_green_node_weights_optimized(abz_ctx* ctx, int n, int npt, PlaneView E, PlaneView W, const double* z_host, int nz) {
    if (E.tile > INT32_MAX || (int64_t)npt * npt > INT32_MAX) {
        set_error("abz_rule_ltm_green_node_weights_optimized: a stride of %lld doubles between grid lines does not fit the kernel's 32-bit "
                  "factor", (long long)E.tile);
        return ABZ_ERR_UNSUPPORTED;
    }
    OptWArgs a;
    a.E = E;
    a.W = W;
    a.npt = npt;
    a.n = n;
    a.weight = 1.0 / (24.0 * (double)npt * (double)npt * (double)npt);
    const int64_t mb = abz_switch(SW_LTM_OPTW_CHUNK_MB) > 0 ? abz_switch(SW_LTM_OPTW_CHUNK_MB) : 256;
    const int64_t cells = (int64_t)npt * npt;  // of a plane
    size_t need = 0;
    for (int cnt : {1, 2})
        if (cnt == 1 ? (green_opt_nodew_nz() == 1 || nz % 2 != 0) : (green_opt_nodew_nz() == 2 && nz >= 2))
            need = std::max(need, sizeof(double) * 24 * (size_t)n * (size_t)(2 * cnt) *
                                      (size_t)optw_planes_of(npt, optw_slab(npt, n, 2 * cnt, mb)) * (size_t)cells);
    const int rc = ctx->scratch[1].reserve(need);
    if (rc) return rc;
    a.C = ctx->scratch[1].as<double>();
    ProfScope ps(ctx, ABZ_K_LTM);
    for (int i0 = 0; i0 < nz;) {
        const int cnt = nz - i0 >= green_opt_nodew_nz() ? green_opt_nodew_nz() : 1;
        for (int i = 0; i < 2; ++i) {
            const int k = i0 + std::min(i, cnt - 1);
            a.Es[2 * i] = z_host[2 * k];
            a.Es[2 * i + 1] = z_host[2 * k + 1];
        }
        a.plane0 = 2 * i0 * n;
        const int S = optw_slab(npt, n, 2 * cnt, mb);
        const bool whole = S + 3 >= npt;
        for (int s0 = 0; s0 < npt; s0 += whole ? npt : S) {
            a.node0 = s0;
            a.nnode = whole ? npt : std::min(S, npt - s0);
            a.nplanes = whole ? npt : a.nnode + 3;
            a.wrap3 = whole;
            a.cell0 = whole ? 0 : (s0 + npt - 2) % npt;  // (S + 3 < npt here: npt >= 5)
            a.wsplane = (int64_t)a.nplanes * cells;
            launch(ctx, GREEN_OPTW_CORNER[cnt == 2], dim3((unsigned)cdiv64(a.wsplane, 256), (unsigned)n), dim3(256), 0, a);
            ABZ_HIP(hipGetLastError());
            launch(ctx, GREEN_OPTW_GATHER[cnt == 2], dim3((unsigned)cdiv64((int64_t)a.nnode * npt * W.row, 256), (unsigned)n), dim3(256), 0, a);
            ABZ_HIP(hipGetLastError());
        }
        i0 += cnt;
    }
    return ABZ_OK;
}

}  // namespace abz
