// Optimized tetrahedron method (gfx950 only): the Green's functions tr G(z) and G_A(z) at complex energies from the effective
// corner values of kernels_ltm_opt.hip (Kawamura, Gohda, Tsuneyuki, PRB 89, 094515 (2014)) and the closed forms of
// kernels_ltm_green.hip.  Both files have the derivations; this one joins them.
//
//  * Definition (d = 3).  For every cell, Kuhn simplex (path v1 -> v2 -> v3 -> v4) and band b: e'_m = sum_j P[m][j] e_b(p_j) over
//    the 20 stencil points of ltm_opt_device.h, with elements A'_{c,m} = sum_j P[m][j] A_{c,b}(p_j): the same P, the same points,
//    the same wrap mod npt (any npt >= 1), the band index followed.  Then
//      tr G(z)  = w sum_{cells} sum_{6 simplices} sum_{bands} J[sort(e'_1 .. e'_4)](z),               w = 1 / (6 npt^3)
//      G_A,c(z) = w sum ...                                  sum_{i=0..3} A'_{c,i} W_i(z),            W_i = J[x_0 .. x_3, x_i](z) / 4
//    by the evaluation rule of ltm_green_device.h as it stands (rho = 1/2, the Taylor series of a narrow sub-range, principal logs
//    of one half plane).  Im z < 0: the conjugate of the value at conj(z), to the bit.
//  * Shape (ltm_green_opt_kernel<SRC, NC>).  The cell walk is ltm_opt_kernel's (blocks of 256 cells, one cell per thread,
//    blockIdx.y the band); the wrapped index tables, the compare-selected stencil (OptPath), the band's planes and the effective
//    elements (opt_elements, here before the z loop) are those of ltm_opt_device.h: nothing indexed by a run-time value.  The
//    simplex loop is the outer one and the loop over z the inner one: the 20 loads and the 4 x 17 product of a simplex (and of
//    each of its NC components) are made once per (cell, simplex, launch) and only the 4 e' and the 4 NC A' of ONE simplex live
//    across the z loop -- 8 + 8 NC VGPRs, where the 24 e' of a cell would take 48 + 48 NC.  The price is that the wave butterfly
//    runs per (simplex, z) instead of per (cell, z): 12 NC shuffle-adds against the 4 log / atan2 pairs, the sort and the closed
//    forms of a simplex, which cannot be shared between the simplices of a cell as the linear kernel shares its 8 corner logs
//    (every simplex has its own four e').  DESIGN section 4e has the register table and the times.
//  * Sources.  OPT_ONE: the trace, green_simplex on the four corners.  OPT_ENERGY: A' = e', nothing loaded.  OPT_ELEMS: NC = 1, 2
//    or 4 components per launch, 20 loads and one product per component.  The last two sort the corners with their A'
//    (green_wsimplex) and contract the four corner weights of a (simplex, z) with every component.
//  * Reduction, as in ltm_green_kernel.  Per (simplex, z) in a fixed order: a butterfly over the wave, lane 0 adds into the wave's
//    LDS slot [zn][NC][re, im] in program order, the four waves are summed in a fixed order into transposed partials and
//    launch_ltm_final finishes.  No atomics: two calls return the same bits, and a z gets the same bits wherever it stands in the
//    list.  A lane beyond the last cell walks cell 0 and adds zeros.  blockIdx.z splits the values of z of a launch where the
//    cells alone do not fill the device.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <vector>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_green_device.h"
#include "ltm_opt_device.h"

namespace abz {

namespace {

struct GreenOptArgs : OptScanArgs {
    const double* z;  // device [nz][2]: re, im > 0
    int nz;
    int zper;         // values of z per blockIdx.z
};

// partial [2 NC nz][nrows]: column (i NC + c) 2 + {0, 1} the real and imaginary part of component c's sum at z_i
template <int SRC, int NC>
__global__ __launch_bounds__(256) void ltm_green_opt_kernel(GreenOptArgs a, double* __restrict__ partial, int64_t nrows) {
    static_assert(SRC == OPT_ELEMS || NC == 1, "one component without attached elements");
    // [zn][2] this block's values of z | [4 waves][zn][NC][2] sums
    extern __shared__ __attribute__((aligned(16))) double ldsgo[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int z0 = (int)blockIdx.z * a.zper;
    const int zn = min(a.zper, a.nz - z0);
    const double* const zl = ldsgo;
    double* const acc = ldsgo + (size_t)2 * zn * (1 + NC * wave);
    for (int i = threadIdx.x; i < 2 * zn; i += 256) ldsgo[i] = a.z[2 * z0 + i];
    for (int i = threadIdx.x; i < 8 * NC * zn; i += 256) ldsgo[2 * zn + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const OptBand<SRC> band(a);
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        const bool active = k < a.ncell;  // (the whole wave takes part in every butterfly)
        const LtmCell cell = ltm_cell<3>(active ? k : 0, npt);
        int j1[4], j2[4], j3[4];
        opt_tables(cell.i1, cell.i2, cell.i3, npt, j1, j2, j3);
#pragma unroll 1
        for (int t = 0; t < 6; ++t) {
            const OptPath path(t, j1, j2, j3);
            double x[OPT_NPT], e[4];
            path.load(band.Eb, band.tileE, x);
            opt_project(x, e);
            [[maybe_unused]] LtmVec<NC> A[4];  // (the trace reads none)
            opt_elements<SRC, NC>(path, band, e, A);
            for (int iz = 0; iz < zn; ++iz) {
                const double zr = zl[2 * iz], zi = zl[2 * iz + 1];
                // the 4 complex logs of z - e'_m: no two simplices of a cell share a corner value
                GreenCorner g[4];
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const double ur = zr - e[m];
                    g[m] = {e[m], 0.5 * log(ur * ur + zi * zi), atan2(zi, ur)};
                }
                double sr[NC], si[NC];
#pragma unroll
                for (int c = 0; c < NC; ++c) sr[c] = si[c] = 0.0;
                if constexpr (SRC == OPT_ONE) {
                    const Cx J = green_simplex(g[0], g[1], g[2], g[3], zr, zi);
                    sr[0] = J.re;
                    si[0] = J.im;
                } else {
                    GreenWCorner<NC> q[4] = {{g[0], A[0]}, {g[1], A[1]}, {g[2], A[2]}, {g[3], A[3]}};
                    green_wsimplex<4, NC>(q, zr, zi, sr, si);
                }
                // every lane ends with the same bits: a + b == b + a at every level of the butterfly
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    sr[c] = active ? sr[c] : 0.0;
                    si[c] = active ? si[c] : 0.0;
#pragma unroll
                    for (int off = 32; off > 0; off >>= 1) {
                        sr[c] += __shfl_xor(sr[c], off);
                        si[c] += __shfl_xor(si[c], off);
                    }
                    if (lane == 0) {
                        acc[2 * (iz * NC + c)] += sr[c];
                        acc[2 * (iz * NC + c) + 1] += si[c];
                    }
                }
            }
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = ldsgo + 2 * zn;
    const size_t w = (size_t)2 * NC * zn;  // from one wave's sums to the next
    for (int t = threadIdx.x; t < 2 * NC * zn; t += 256)
        partial[((int64_t)2 * NC * z0 + t) * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
}

using GreenOptFn = void (*)(abz_ctx*, dim3, size_t, const GreenOptArgs&, double*, int64_t);
template <int SRC, int NC>
void green_opt_launch(abz_ctx* ctx, dim3 grid, size_t lds, const GreenOptArgs& a, double* partial, int64_t nrows) {
    launch(ctx, (ltm_green_opt_kernel<SRC, NC>), grid, dim3(256), (unsigned)lds, a, partial, nrows);
}

// the compiled kernels: [source][NC]
GreenOptFn green_opt_fn(int src, int nc) {
    if (src == OPT_ONE) return green_opt_launch<OPT_ONE, 1>;
    if (src == OPT_ENERGY) return green_opt_launch<OPT_ENERGY, 1>;
    switch (nc) {
        case 1: return green_opt_launch<OPT_ELEMS, 1>;
        case 2: return green_opt_launch<OPT_ELEMS, 2>;
        case 4: return green_opt_launch<OPT_ELEMS, 4>;
    }
    return nullptr;
}

}  // namespace

// The host side of ltm_green_scan (kernels_ltm_green.hip) for the optimized kernel: the same chunks of z, groups of 4, 2, 1
// components, mailbox delivery and sign of Im z < 0; ltm_green_scan is internal to its file, which keeps its object code.
// A == nullptr: one component, the trace (`energy` false) or A' = e' (`energy` true).  z_host [nz][2] with Im z != 0, out_host
// [nz][ncomp][2].
int launch_ltm_green_optimized(abz_ctx* ctx, int n, int npt, PlaneView E, const PlaneView* A, bool energy, int ncomp, const double* z_host, int nz,
                               double* out_host) {
    GreenOptArgs a{};
    int src;
    int64_t nblocks, nrows;
    int rc = opt_scan_open("abz_rule_ltm_green_optimized", n, npt, E, A, energy, ncomp, a, src, nblocks, nrows);
    if (rc) return rc;
    // of a simplex and, with elements, of its 4 corner weights the 1 / 4
    const double weight = 1.0 / (6.0 * (double)a.ncell * (src == OPT_ONE ? 1.0 : 4.0));
    std::vector<double> zup(2 * (size_t)nz);
    for (size_t i = 0; i < (size_t)nz; ++i) {
        zup[2 * i] = z_host[2 * i];
        zup[2 * i + 1] = std::fabs(z_host[2 * i + 1]);
    }
    size_t pmax = 0;
    for (int nc : {1, 2, 4})
        if (nc <= ncomp) pmax = std::max(pmax, (size_t)std::min(nz, green_w_chunk(nc)) * (size_t)(2 * nc));
    if ((rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nrows * pmax))) return rc;
    double* partial = ctx->scratch[1].as<double>();
    const double* zdev = nullptr;
    if ((rc = sweep_to_device(ctx, zup.data(), 2 * nz, &zdev))) return rc;
    const size_t ncols = (size_t)nz * (size_t)ncomp;
    const SumOut so = sum_out_mailbox(ctx, out_host, ncols);
    double2* where = nullptr;
    if ((rc = sum_target(ctx, so, 0, (int64_t)ncols, &where))) return rc;
    for (int c0 = 0; c0 < ncomp;) {
        const int nc = ncomp - c0 >= 4 ? 4 : (ncomp - c0 >= 2 ? 2 : 1);
        const int CH = green_w_chunk(nc);
        const GreenOptFn fn = green_opt_fn(src, nc);
        a.aplane0 = c0 * n;
        for (int s0 = 0; s0 < nz; s0 += CH) {
            const int cnt = std::min(CH, nz - s0);
            // where the cells give fewer than ~2048 blocks the values of z are dealt to blockIdx.z, at least 4 per block
            const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(2048, nrows), cdiv64(cnt, 4)));
            a.z = zdev + 2 * (size_t)s0;
            a.nz = cnt;
            a.zper = (int)cdiv64(cnt, nsplit);
            const dim3 grid((unsigned)nblocks, (unsigned)n, (unsigned)cdiv64(cnt, a.zper));
            ProfScope ps(ctx, ABZ_K_LTM);
            fn(ctx, grid, sizeof(double) * (size_t)(2 + 8 * nc) * (size_t)a.zper, a, partial, nrows);
            ABZ_HIP(hipGetLastError());
            // column (i nc + c) 2 + t of the launch -> out[s0 + i][c0 + c][t]
            if ((rc = launch_ltm_final(ctx, partial, nrows, weight, 2 * nc * cnt, 2 * nc, 2 * ncomp,
                                       reinterpret_cast<double*>(where + ((size_t)s0 * (size_t)ncomp + (size_t)c0)))))
                return rc;
        }
        c0 += nc;
    }
    if ((rc = sum_deliver(ctx, so, where, 0, (int64_t)ncols))) return rc;
    for (size_t i = 0; i < (size_t)nz; ++i)
        if (z_host[2 * i + 1] < 0.0)
            for (size_t c = 0; c < (size_t)ncomp; ++c) out_host[2 * (i * (size_t)ncomp + c) + 1] = -out_host[2 * (i * (size_t)ncomp + c) + 1];
    return ABZ_OK;
}

}  // namespace abz
