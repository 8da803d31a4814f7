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
//    A'. ltm_green_opt_cornerw_kernel<NZ>: the cell walk of ltm_opt_cornerw_kernel (optw_cell: one cell per thread, blockIdx.y the
//       band) and the stencil addressing OptPath of ltm_opt_device.h (the six simplices under unroll 1, nothing indexed at run
//       time, a 32-bit line stride that the host checks).  Per simplex 20 loads, opt_project, the five-step compare-exchange sort
//       that carries each corner's path position (optw_sort), the four corner logs (taken after the sort), green_weights<4> per z, and 8 NZ stores in path order into the
//       workspace [band][set][t 4 + m][cell] as 2 NZ real sets: set 2 iz = Re, set 2 iz + 1 = Im with the sign of Im z applied.
//       Every simplex stores: the workspace needs no clearing.
//    B. ltm_opt_nodew_gather_kernel<2 NZ> (ltm_opt_nodew_device.h), the gather of the real weights as it is: it sums the 432 terms
//       of a node per set in one fixed order (t, j, m) and writes plane (plane0 / n + set) n + b, which is the layout of the complex
//       block.  The host's scale is 1 / (24 npt^3): of a simplex, and of its corner weights the 1 / 4.
//  * Workspace and slabs: scratch[1] under ABZ_LTM_OPTW_CHUNK_MB, the slab planner and the slab loop of the real weights
//    (optw_need, optw_run_group of ltm_opt_nodew_device.h) for 2 NZ sets.  A node's terms and their order do not depend on the slab height: the block has the same bits for every cap.
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
    const OptWCell c = optw_cell(a, kk, 2 * NZ);  // (a value of z is two sets: Re, Im)
    double zr[NZ], zi[NZ];
    bool neg[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        zr[i] = a.Es[2 * i];
        zi[i] = fabs(a.Es[2 * i + 1]);
        neg[i] = a.Es[2 * i + 1] < 0.0;
    }
#pragma unroll 1
    for (int t = 0; t < 6; ++t) {
        const OptPath path(t, c.j1, c.j2, c.j3);
        double x[OPT_NPT], e[4];
        path.load(c.Eb, c.tileE, x);
        opt_project(x, e);
        const OptWSorted s = optw_sort(e);
        const double e1 = s.e1, e2 = s.e2, e3 = s.e3, e4 = s.e4;
        double* __restrict__ const ot = c.out + (int64_t)(t * 4) * a.wsplane;
#pragma unroll
        for (int i = 0; i < NZ; ++i) {
            const double u1 = zr[i] - e1, u2 = zr[i] - e2, u3 = zr[i] - e3, u4 = zr[i] - e4, y = zi[i];
            const GreenCorner g[4] = {{e1, 0.5 * log(u1 * u1 + y * y), atan2(y, u1)},
                                      {e2, 0.5 * log(u2 * u2 + y * y), atan2(y, u2)},
                                      {e3, 0.5 * log(u3 * u3 + y * y), atan2(y, u3)},
                                      {e4, 0.5 * log(u4 * u4 + y * y), atan2(y, u4)}};
            Cx W[4];
            green_weights<4>(g, zr[i], y, W);
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const double im = optw_of_path(s, m, W[0].im, W[1].im, W[2].im, W[3].im);
                ot[(int64_t)((2 * i) * 24 + m) * a.wsplane] = optw_of_path(s, m, W[0].re, W[1].re, W[2].re, W[3].re);
                ot[(int64_t)((2 * i + 1) * 24 + m) * a.wsplane] = neg[i] ? -im : im;
            }
        }
    }
}

// Values of z per group where at least that many remain.  A' is the expensive kernel and the slab overlap (S + 3) / S multiplies
// it: a pair takes 4 sets and gets shorter slabs under the cap than a single value's 2 sets.  Measured at SVO 150^3 under the default
// cap: 39.6 ms per z alone, 47.7 ms in pairs; where one slab holds the grid the pair is 1.47 times faster.
#ifndef ABZ_LTM_GREEN_OPTW_NZ
#define ABZ_LTM_GREEN_OPTW_NZ 1
#endif
constexpr int green_opt_nodew_nz() { return ABZ_LTM_GREEN_OPTW_NZ; }
static_assert(green_opt_nodew_nz() == 1 || green_opt_nodew_nz() == 2, "a group is one value of z or a pair");

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
    size_t need = 0;
    for (int cnt : {1, 2})
        if (cnt == 1 ? (green_opt_nodew_nz() == 1 || nz % 2 != 0) : (green_opt_nodew_nz() == 2 && nz >= 2))
            need = std::max(need, optw_need(npt, n, 2 * cnt));
    int rc = ctx->scratch[1].reserve(need);
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
        if ((rc = optw_run_group(ctx, a, 2 * cnt, GREEN_OPTW_CORNER[cnt == 2], GREEN_OPTW_GATHER[cnt == 2]))) return rc;
        i0 += cnt;
    }
    return ABZ_OK;
}

}  // namespace abz
