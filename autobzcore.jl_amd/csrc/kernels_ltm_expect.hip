// Band expectation values of operator series as matrix elements of the tetrahedron method (abz_rule_ltm_expectation):
//   q_i(b, k) = Re u_b(k)^H Hermitian(O_i(k)) u_b(k),   component c = q_i (single) or q_i q_j (product),
// the H planes of a whole periodic grid and the planes of up to ABZ_LTM_EXPECT_MAX_OPS operator rules of the same grid in,
// the element block of abz_rule_ltm_elements out (plane c n + b of a grid line's tile, padded rows, the padding columns
// written as zeros).  Siblings of the two orbital kernels (kernels_ltm_orb.hip): the same loads of H, the same solves, the
// same stores; neither U nor O u reaches HBM, no atomics, no dependence on the launch geometry: two calls write the same bits.
// Of every operator the upper triangle is read, the way H is read (either plane layout, each rule with its own tiling).
//   1...4 bands   one grid point per lane: herm_eig<N, true>, then per operator its N (N + 1) / 2 upper-triangle entries and
//                 the form sum_p O_pp |u_p|^2 + 2 Re sum_{p<q} conj(u_p) O_pq u_q in registers;
//   5...32 bands  NP = 8 / 16 / 32 lanes per node: after rows_eigh_columns (column b of U in lane b) lane r loads row r of
//                 O_i, the upper triangle is parked in the node's LDS room -- the room of the reflectors, free once the
//                 back-transformation is done -- and lane b forms u_b^H O_i u_b from broadcast reads (quad_form of
//                 rows_eigvec.h, the form of the GGR velocities).  One operator after another: one room.  The nops results
//                 stay in registers (written by select chains: the operator index is uniform but a run-time number, an
//                 index into a register array would be scratch); the components leave through an LDS tile
//                 [component][band][node] as contiguous row segments.
// LDS per workgroup, 16 components: 53 KB (NP = 8), 70 KB (NP = 16: two workgroups per CU), 104 KB (NP = 32: one).
// Registers (the compiler's resource report): no scratch in the lane kernels and at NP = 8.  NP = 16 has 504 B of scratch per
// lane at 256 VGPRs and NP = 32 644 B at 512: the eigen-solve is held to the register budget of two workgroups (one at
// NP = 32) per CU and spills inside the inverse iteration -- the orbital kernel, the same solve, has 352 and 356 B -- and the
// column u_b (2 NP doubles) stays alive beside the operator row being loaded (another 2 NP).  One workgroup per CU at 16 bands
// would end the spills and halve the nodes in flight; the orbital kernel made the same choice.
// At a degenerate level u_b is some orthonormal basis of the eigenspace: the sum of single expectations over the level is
// defined, single values and products are not.
#include <utility>

#include "abz_internal.h"
#include "device_math.h"
#include "rows_device.h"
#include "rows_eigvec.h"
#include "xp_select.h"

namespace abz {

namespace {

constexpr int XOPS = ABZ_LTM_EXPECT_MAX_OPS;

struct LtmExpectArgs {
    PlaneView H;        // H planes of the grid (full or Hermitian-compact); unused for one band
    PlaneView O[XOPS];  // the operators' planes, each in its own layout and tiling
    PlaneView A;        // the element block: ncomp n planes, tiled like the eigenvalue planes
    int64_t nlines;
    int n, npt, nops, ncomp;
    int ci[ABZ_LTM_MAX_COMP], cj[ABZ_LTM_MAX_COMP];  // component c: q[ci] (cj < 0) or q[ci] q[cj]
};

template <int N>
__global__ __launch_bounds__(256) void ltm_expect_lane_kernel(LtmExpectArgs a) {
    const int row = a.A.row;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t / row;
    const int i = (int)(t - line * row);
    double q[N][XOPS];  // [band][operator]; zeros in the padding columns
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int k = 0; k < XOPS; ++k) q[b][k] = 0.0;
    }
    if (i < a.npt) {
        CMat<N> V;
        if constexpr (N == 1) {
            V.re[0][0] = 1.0;
            V.im[0][0] = 0.0;
        } else {
            const double* __restrict__ const in = a.H.base + line * a.H.tile + i;
            CMat<N> h;
#pragma unroll
            for (int p = 0; p < N; ++p) {
#pragma unroll
                for (int s = 0; s < N; ++s) {
                    h.re[p][s] = 0.0;
                    h.im[p][s] = 0.0;
                    if (p <= s) {
                        const int64_t pl = xp_plane(a.H, N, p, s);
                        h.re[p][s] = in[pl * a.H.pitch];
                        if (p < s) h.im[p][s] = in[(pl + 1) * a.H.pitch];
                    }
                }
            }
            double e[N];
            herm_eig<N, true>(h, e, V);
        }
        for (int k = 0; k < a.nops; ++k) {  // (uniform)
            const PlaneView& O = a.O[k];
            const double* __restrict__ const in = O.base + line * O.tile + i;
            double v[N];
#pragma unroll
            for (int b = 0; b < N; ++b) v[b] = 0.0;
#pragma unroll
            for (int s = 0; s < N; ++s) {
#pragma unroll
                for (int p = 0; p <= s; ++p) {
                    const int64_t pl = xp_plane(O, N, p, s);
                    const double ore = in[pl * O.pitch];
                    if (p == s) {
#pragma unroll
                        for (int b = 0; b < N; ++b) v[b] = fma(ore, fma(V.re[p][b], V.re[p][b], V.im[p][b] * V.im[p][b]), v[b]);
                    } else {
                        const double oim = in[(pl + 1) * O.pitch];
#pragma unroll
                        for (int b = 0; b < N; ++b) {
                            const double tr = fma(V.re[p][b], V.re[s][b], V.im[p][b] * V.im[s][b]);  // conj(u_p) u_s
                            const double ti = fma(V.re[p][b], V.im[s][b], -V.im[p][b] * V.re[s][b]);
                            v[b] = fma(2.0, fma(ore, tr, -oim * ti), v[b]);
                        }
                    }
                }
            }
#pragma unroll
            for (int b = 0; b < N; ++b) xp_put(q[b], k, v[b]);
        }
    }
    double* __restrict__ const out = a.A.base + line * a.A.tile + i;
    for (int c = 0; c < a.ncomp; ++c) {
        const int ki = a.ci[c], kj = a.cj[c];  // (uniform)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            const double x = xp_pick(q[b], ki);
            out[(int64_t)(c * N + b) * a.A.pitch] = kj < 0 ? x : x * xp_pick(q[b], kj);
        }
    }
}

template <int NP>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ltm_expect_rows_kernel(LtmExpectArgs a) {
    extern __shared__ double2 lds_xp[];
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    const int slot = threadIdx.x / NP, r0 = threadIdx.x % NP, lane = threadIdx.x & 63;
    double2* const park = lds_xp + (size_t)slot * PARK_STRIDE<NP>;                     // this node's reflectors, then its operator
    double* const tile = reinterpret_cast<double*>(lds_xp + SLOTS * PARK_STRIDE<NP>);  // [component][NP bands][TS]
    const int npt = a.npt, nplanes = a.ncomp * a.n;
    const int ppl = (npt + SLOTS - 1) / SLOTS;  // passes per line
    for (int64_t item = blockIdx.x; item < a.nlines * ppl; item += gridDim.x) {
        const int64_t line = item / ppl;
        const int i0 = (int)(item - line * ppl) * SLOTS;
        // (see ggr_rows_kernel: what depends on n and r alone must not be hoisted out of the loop and kept alive through it)
        int n = a.n, r = r0;
        asm volatile("" : "+s"(n));
        asm volatile("" : "+v"(r));
        const bool wave_on = i0 + (int)(threadIdx.x >> 6) * (64 / NP) < npt;  // a wave without a node keeps the barriers only
        const int i1 = i0 + slot;
        const bool act = i1 < npt;
        if (wave_on) {
            const int rr = r < n ? r : n - 1;
            double hr[NP], hi[NP];
            // row r of Hermitian(X): (r, j) of the upper triangle for j >= r, the conjugate of (j, r) below the diagonal
            auto load_row = [&](const PlaneView& X) {
                const double* __restrict__ const in = X.base + line * X.tile + (act ? i1 : 0);
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    hr[j] = 0.0;
                    hi[j] = 0.0;
                    if (j < n) {  // uniform
                        const int lo = rr < j ? rr : j, up = rr < j ? j : rr;
                        const int64_t pl = xp_plane(X, n, lo, up);
                        const double re = in[pl * X.pitch];
                        const double im = in[(pl + (lo != up ? 1 : 0)) * X.pitch];
                        hr[j] = r < n ? re : 0.0;
                        hi[j] = (r < n && lo != up) ? (rr < j ? im : -im) : 0.0;
                    }
                }
            };
            load_row(a.H);
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, lane, park, hr, hi, myeig, ur, ui);
            double q[XOPS];
#pragma unroll
            for (int m = 0; m < XOPS; ++m) q[m] = 0.0;
            for (int k = 0; k < a.nops; ++k) {  // (uniform)
                load_row(a.O[k]);
                wave_sync_lds();  // every lane of the node is done reading the room (reflectors, the operator before)
                park_upper<NP>(n, r, park, hr, hi);
                wave_sync_lds();
                const double v = quad_form<NP>(n, park, ur, ui, std::make_integer_sequence<int, NP>());
                xp_put(q, k, v);
            }
            if (act && r < n) {
                for (int c = 0; c < a.ncomp; ++c) {
                    const int ki = a.ci[c], kj = a.cj[c];  // (uniform)
                    const double x = xp_pick(q, ki);
                    tile[(c * NP + r) * TS + slot] = kj < 0 ? x : x * xp_pick(q, kj);
                }
            }
        }
        __syncthreads();
        // the pass's columns of every plane; the line's last pass takes the padding columns along, as zeros
        const int width = (i0 + SLOTS >= npt) ? a.A.row - i0 : SLOTS;
        double* __restrict__ const out = a.A.base + line * a.A.tile + i0;
        for (int idx = threadIdx.x; idx < nplanes * width; idx += 256) {
            const int pl = idx / width, sl = idx - pl * width;
            const int c = pl / a.n, b = pl - c * a.n;
            out[(int64_t)pl * a.A.pitch + sl] = (i0 + sl < npt) ? tile[(c * NP + b) * TS + sl] : 0.0;
        }
        __syncthreads();  // the tile is free for the next pass
    }
}

size_t ltm_expect_lds_bytes(int np, int ncomp) {
    const size_t slots = (size_t)(256 / np);
    return sizeof(double2) * slots * (size_t)(np * (np + 1) / 2 + 1) + sizeof(double) * (size_t)ncomp * np * (slots + 1);
}

}  // namespace

int launch_ltm_expectation(abz_ctx* ctx, int n, int npt, int64_t nlines, PlaneView H, const PlaneView* ops, int nops, PlaneView A,
                           const int32_t* comps, int ncomp) {
    if (nlines <= 0) return ABZ_OK;
    LtmExpectArgs a;
    a.H = H;
    a.A = A;
    a.nlines = nlines;
    a.n = n;
    a.npt = npt;
    a.nops = nops;
    a.ncomp = ncomp;
    for (int k = 0; k < XOPS; ++k) a.O[k] = ops[k < nops ? k : 0];
    for (int c = 0; c < ABZ_LTM_MAX_COMP; ++c) {
        a.ci[c] = c < ncomp ? (comps ? comps[2 * c] : c) : 0;
        a.cj[c] = c < ncomp ? (comps ? comps[2 * c + 1] : -1) : -1;
    }
    ProfScope ps(ctx, ABZ_K_EIG);
    if (n <= 4) {
        const dim3 grid((unsigned)((nlines * A.row + 255) / 256));
        switch (n) {
            case 1: launch(ctx, ltm_expect_lane_kernel<1>, grid, dim3(256), 0, a); break;
            case 2: launch(ctx, ltm_expect_lane_kernel<2>, grid, dim3(256), 0, a); break;
            case 3: launch(ctx, ltm_expect_lane_kernel<3>, grid, dim3(256), 0, a); break;
            default: launch(ctx, ltm_expect_lane_kernel<4>, grid, dim3(256), 0, a); break;
        }
    } else {
        const int np = n <= 8 ? 8 : (n <= 16 ? 16 : 32);
        const size_t lds = ltm_expect_lds_bytes(np, ncomp);
        const int64_t blocks = std::min<int64_t>(nlines * ((npt + 256 / np - 1) / (256 / np)), 256 * 64);
#define ABZ_LX(NPV)                                                                                                              \
    {                                                                                                                            \
        ABZ_HIP(hipFuncSetAttribute((const void*)ltm_expect_rows_kernel<NPV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        launch(ctx, (ltm_expect_rows_kernel<NPV>), dim3((unsigned)blocks), dim3(256), lds, a);                                   \
    }
        if (np == 8) ABZ_LX(8)
        else if (np == 16) ABZ_LX(16)
        else ABZ_LX(32)
#undef ABZ_LX
    }
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
