// Orbital weights |U_ab(k)|^2 as matrix elements of the tetrahedron method (abz_rule_ltm_orbitals): the H planes of a whole
// periodic grid in, the element block of abz_rule_ltm_elements out -- plane c n + b of a grid line's tile = component c
// (orbital orb[c]) of band b, padded rows, the padding columns written as zeros -- with nothing in between: no U in HBM, no
// host.  U(k) = orthonormal eigenvectors of Hermitian(H(k)), the upper triangle (either H layout holds it: the same numbers
// reach the solver), bands ascending as in the rule's eigenvalue planes.
//   1...4 bands   one grid point per lane (the columns of a padded row: a wave's stores are whole 128-B segments straight
//                 from registers), cyclic Jacobi with accumulated rotations and the sorting network of herm_eig<N, true>;
//   5...32 bands  the row layout of the GGR build, NP = 8 / 16 / 32 lanes per node: lane r loads row r, rows_eigh_columns
//                 (rows_eigvec.h: kept Householder reflectors, bisection, tridiagonal inverse iteration with cluster
//                 re-orthogonalisation, back-transformation) leaves column b of U in lane b, the squared moduli of the
//                 selected orbitals go to an LDS tile [orbital][band][node] and leave as contiguous row segments.
// Degenerate levels get some orthonormal basis of their eigenspace (the contract of the GGR build and of the reference,
// src/dos_ggr.jl:31-44): sums over the level and both normalisations are defined, single weights are not.  No atomics, no
// dependence on the launch geometry: two calls write the same bits.
// The band projectors U_pb conj(U_qb) of abz_rule_ltm_projectors (second half of the file) come from sibling kernels with the
// same loads, solves and stores.
#include <utility>

#include "abz_internal.h"
#include "device_math.h"
#include "rows_device.h"
#include "rows_eigvec.h"

namespace abz {

namespace {

struct LtmOrbArgs {
    PlaneView H;  // H planes of the grid (full or Hermitian-compact)
    PlaneView A;  // the element block: ncomp n planes, tiled like the eigenvalue planes
    int64_t nlines;
    int n, npt, ncomp;
    unsigned mask;  // bit a: orbital a is asked for
    int orb[ABZ_LTM_MAX_COMP];
};

// plane of Re H[a][b], a <= b (Im: the next one; the diagonal of the compact layout has none)
__device__ __forceinline__ int orb_hplane(const PlaneView& v, int n, int a, int b) { return v.compact ? b * b + 2 * a : 2 * (a + n * b); }

template <int N>
__global__ __launch_bounds__(256) void ltm_orb_lane_kernel(LtmOrbArgs a) {
    const int row = a.A.row;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t / row;
    const int i = (int)(t - line * row);
    double w[N][N];  // [orbital][band]
#pragma unroll
    for (int o = 0; o < N; ++o) {
#pragma unroll
        for (int b = 0; b < N; ++b) w[o][b] = 0.0;
    }
    if (i < a.npt) {
        if constexpr (N == 1) {
            w[0][0] = 1.0;
        } else {
            const double* __restrict__ const in = a.H.base + line * a.H.tile + i;
            CMat<N> h, V;
#pragma unroll
            for (int p = 0; p < N; ++p) {
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    h.re[p][q] = 0.0;
                    h.im[p][q] = 0.0;
                    if (p <= q) {
                        const int64_t pl = orb_hplane(a.H, N, p, q);
                        h.re[p][q] = in[pl * a.H.pitch];
                        if (p < q) h.im[p][q] = in[(pl + 1) * a.H.pitch];
                    }
                }
            }
            double e[N];
            herm_eig<N, true>(h, e, V);
#pragma unroll
            for (int o = 0; o < N; ++o) {
#pragma unroll
                for (int b = 0; b < N; ++b) w[o][b] = fma(V.re[o][b], V.re[o][b], V.im[o][b] * V.im[o][b]);
            }
        }
    }
    double* __restrict__ const out = a.A.base + line * a.A.tile + i;
    for (int c = 0; c < a.ncomp; ++c) {
        const int o = a.orb[c];  // (uniform)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double v = w[0][b];
#pragma unroll
            for (int p = 1; p < N; ++p) v = (o == p) ? w[p][b] : v;
            out[(int64_t)(c * N + b) * a.A.pitch] = v;
        }
    }
}

template <int NP>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ltm_orb_rows_kernel(LtmOrbArgs a) {
    extern __shared__ double2 lds_orb[];
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    const int slot = threadIdx.x / NP, r0 = threadIdx.x % NP, lane = threadIdx.x & 63;
    double2* const park = lds_orb + (size_t)slot * PARK_STRIDE<NP>;                        // this node's reflectors
    double* const tile = reinterpret_cast<double*>(lds_orb + SLOTS * PARK_STRIDE<NP>);  // [asked orbital][NP bands][TS]
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
            // row r of Hermitian(H): (r, j) of the upper triangle for j >= r, the conjugate of (j, r) below the diagonal
            const double* __restrict__ const in = a.H.base + line * a.H.tile + (act ? i1 : 0);
            const int rr = r < n ? r : n - 1;
            double hr[NP], hi[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                hr[j] = 0.0;
                hi[j] = 0.0;
                if (j < n) {  // uniform
                    const int lo = rr < j ? rr : j, up = rr < j ? j : rr;
                    const int64_t pl = orb_hplane(a.H, n, lo, up);
                    const double re = in[pl * a.H.pitch];
                    const double im = in[(pl + (lo != up ? 1 : 0)) * a.H.pitch];
                    hr[j] = r < n ? re : 0.0;
                    hi[j] = (r < n && lo != up) ? (rr < j ? im : -im) : 0.0;
                }
            }
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, lane, park, hr, hi, myeig, ur, ui);
            if (act && r < n) {
                int rank = 0;  // position of orbital o among the asked ones
#pragma unroll
                for (int o = 0; o < NP; ++o) {
                    if (o < n && ((a.mask >> o) & 1u)) {  // uniform
                        tile[(rank * NP + r) * TS + slot] = fma(ur[o], ur[o], ui[o] * ui[o]);
                        ++rank;
                    }
                }
            }
        }
        __syncthreads();
        // the pass's columns of every plane; the line's last pass takes the padding columns along, as zeros
        const int width = (i0 + SLOTS >= npt) ? a.A.row - i0 : SLOTS;
        double* __restrict__ const out = a.A.base + line * a.A.tile + i0;
        for (int idx = threadIdx.x; idx < nplanes * width; idx += 256) {
            const int pl = idx / width, sl = idx - pl * width;
            const int c = pl / n, b = pl - c * n;
            const int rank = __popc(a.mask & ((1u << a.orb[c]) - 1u));
            out[(int64_t)pl * a.A.pitch + sl] = (i0 + sl < npt) ? tile[(rank * NP + b) * TS + sl] : 0.0;
        }
        __syncthreads();  // the tile is free for the next pass
    }
}

// ---- band projectors P^b_pq(k) = U_pb conj(U_qb) (abz_rule_ltm_projectors) ---------------------------------------------------
// Siblings of the two kernels above with the same loads, the same eigen-solves and the same stores; what differs is the
// product formed from column b of U.  Pair i = (p[i], q[i]) fills components c0[i] (p == q: |U_pb|^2, the expression of the
// orbital weights, bit for bit) or c0[i], c0[i] + 1 (p != q: Re and Im of the projector).  The phase of an eigenvector
// cancels in the product, so no gauge is fixed anywhere.  p and q are uniform but known at run time only: the values are
// picked by unrolled select chains (an index into a register array would be scratch).
struct LtmProjArgs {
    PlaneView H, A;
    int64_t nlines;
    int n, npt, npairs, ncomp;
    int p[ABZ_LTM_MAX_COMP], q[ABZ_LTM_MAX_COMP], c0[ABZ_LTM_MAX_COMP];
};

// x[o] of a register array into v, o uniform (as in ltm_orb_lane_kernel: written where it is used, on the array itself)
#define ABZ_PICK(v, x, o, N)                            \
    double v = (x)[0];                                  \
    _Pragma("unroll") for (int j_ = 1; j_ < (N); ++j_) v = ((o) == j_) ? (x)[j_] : v;

__device__ __forceinline__ double proj_diag(double re, double im) { return fma(re, re, im * im); }
__device__ __forceinline__ double proj_re(double pr, double pi, double qr, double qi) { return fma(pr, qr, pi * qi); }
__device__ __forceinline__ double proj_im(double pr, double pi, double qr, double qi) { return fma(pi, qr, -(pr * qi)); }

template <int N>
__global__ __launch_bounds__(256) void ltm_proj_lane_kernel(LtmProjArgs a) {
    const int row = a.A.row;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t / row;
    const int i = (int)(t - line * row);
    double ur[N][N], ui[N][N];  // [band][orbital]; zeros in the padding columns
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int o = 0; o < N; ++o) ur[b][o] = ui[b][o] = 0.0;
    }
    if (i < a.npt) {
        if constexpr (N == 1) {
            ur[0][0] = 1.0;
        } else {
            const double* __restrict__ const in = a.H.base + line * a.H.tile + i;
            CMat<N> h, V;
#pragma unroll
            for (int p = 0; p < N; ++p) {
#pragma unroll
                for (int q = 0; q < N; ++q) {
                    h.re[p][q] = 0.0;
                    h.im[p][q] = 0.0;
                    if (p <= q) {
                        const int64_t pl = orb_hplane(a.H, N, p, q);
                        h.re[p][q] = in[pl * a.H.pitch];
                        if (p < q) h.im[p][q] = in[(pl + 1) * a.H.pitch];
                    }
                }
            }
            double e[N];
            herm_eig<N, true>(h, e, V);
#pragma unroll
            for (int b = 0; b < N; ++b) {
#pragma unroll
                for (int o = 0; o < N; ++o) {
                    ur[b][o] = V.re[o][b];
                    ui[b][o] = V.im[o][b];
                }
            }
        }
    }
    double* __restrict__ const out = a.A.base + line * a.A.tile + i;
    for (int k = 0; k < a.npairs; ++k) {
        const int p = a.p[k], q = a.q[k], c = a.c0[k];  // (uniform)
#pragma unroll
        for (int b = 0; b < N; ++b) {
            ABZ_PICK(pr, ur[b], p, N)
            ABZ_PICK(pi, ui[b], p, N)
            if (p == q) {
                out[(int64_t)(c * N + b) * a.A.pitch] = proj_diag(pr, pi);
            } else {
                ABZ_PICK(qr, ur[b], q, N)
                ABZ_PICK(qi, ui[b], q, N)
                out[(int64_t)(c * N + b) * a.A.pitch] = proj_re(pr, pi, qr, qi);
                out[(int64_t)((c + 1) * N + b) * a.A.pitch] = proj_im(pr, pi, qr, qi);
            }
        }
    }
}

template <int NP>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ltm_proj_rows_kernel(LtmProjArgs a) {
    extern __shared__ double2 lds_orb[];
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    const int slot = threadIdx.x / NP, r0 = threadIdx.x % NP, lane = threadIdx.x & 63;
    double2* const park = lds_orb + (size_t)slot * PARK_STRIDE<NP>;                        // this node's reflectors
    double* const tile = reinterpret_cast<double*>(lds_orb + SLOTS * PARK_STRIDE<NP>);  // [component][NP bands][TS]
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
            // row r of Hermitian(H): (r, j) of the upper triangle for j >= r, the conjugate of (j, r) below the diagonal
            const double* __restrict__ const in = a.H.base + line * a.H.tile + (act ? i1 : 0);
            const int rr = r < n ? r : n - 1;
            double hr[NP], hi[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                hr[j] = 0.0;
                hi[j] = 0.0;
                if (j < n) {  // uniform
                    const int lo = rr < j ? rr : j, up = rr < j ? j : rr;
                    const int64_t pl = orb_hplane(a.H, n, lo, up);
                    const double re = in[pl * a.H.pitch];
                    const double im = in[(pl + (lo != up ? 1 : 0)) * a.H.pitch];
                    hr[j] = r < n ? re : 0.0;
                    hi[j] = (r < n && lo != up) ? (rr < j ? im : -im) : 0.0;
                }
            }
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, lane, park, hr, hi, myeig, ur, ui);
            if (act && r < n) {
                for (int k = 0; k < a.npairs; ++k) {
                    const int p = a.p[k], q = a.q[k], c = a.c0[k];  // (uniform)
                    ABZ_PICK(pr, ur, p, NP)
                    ABZ_PICK(pi, ui, p, NP)
                    if (p == q) {
                        tile[(c * NP + r) * TS + slot] = proj_diag(pr, pi);
                    } else {
                        ABZ_PICK(qr, ur, q, NP)
                        ABZ_PICK(qi, ui, q, NP)
                        tile[(c * NP + r) * TS + slot] = proj_re(pr, pi, qr, qi);
                        tile[((c + 1) * NP + r) * TS + slot] = proj_im(pr, pi, qr, qi);
                    }
                }
            }
        }
        __syncthreads();
        // the pass's columns of every plane; the line's last pass takes the padding columns along, as zeros
        const int width = (i0 + SLOTS >= npt) ? a.A.row - i0 : SLOTS;
        double* __restrict__ const out = a.A.base + line * a.A.tile + i0;
        for (int idx = threadIdx.x; idx < nplanes * width; idx += 256) {
            const int pl = idx / width, sl = idx - pl * width;
            const int c = pl / n, b = pl - c * n;
            out[(int64_t)pl * a.A.pitch + sl] = (i0 + sl < npt) ? tile[(c * NP + b) * TS + sl] : 0.0;
        }
        __syncthreads();  // the tile is free for the next pass
    }
}
#undef ABZ_PICK

size_t ltm_orb_lds_bytes(int np, int ndist) {
    const size_t slots = (size_t)(256 / np);
    return sizeof(double2) * slots * (size_t)(np * (np + 1) / 2 + 1) + sizeof(double) * (size_t)ndist * np * (slots + 1);
}

}  // namespace

bool ltm_orbitals_supported(int n) { return n >= 1 && n <= 32; }

int launch_ltm_orbitals(abz_ctx* ctx, int n, int npt, int64_t nlines, PlaneView H, PlaneView A, const int32_t* orb, int ncomp) {
    if (nlines <= 0) return ABZ_OK;
    LtmOrbArgs a;
    a.H = H;
    a.A = A;
    a.nlines = nlines;
    a.n = n;
    a.npt = npt;
    a.ncomp = ncomp;
    a.mask = 0;
    for (int c = 0; c < ABZ_LTM_MAX_COMP; ++c) {
        a.orb[c] = c < ncomp ? (orb ? orb[c] : c) : 0;
        if (c < ncomp) a.mask |= 1u << a.orb[c];
    }
    ProfScope ps(ctx, ABZ_K_EIG);
    if (n <= 4) {
        const dim3 grid((unsigned)((nlines * A.row + 255) / 256));
        switch (n) {
            case 1: launch(ctx, ltm_orb_lane_kernel<1>, grid, dim3(256), 0, a); break;
            case 2: launch(ctx, ltm_orb_lane_kernel<2>, grid, dim3(256), 0, a); break;
            case 3: launch(ctx, ltm_orb_lane_kernel<3>, grid, dim3(256), 0, a); break;
            default: launch(ctx, ltm_orb_lane_kernel<4>, grid, dim3(256), 0, a); break;
        }
    } else {
        const int np = n <= 8 ? 8 : (n <= 16 ? 16 : 32);
        const size_t lds = ltm_orb_lds_bytes(np, __builtin_popcount(a.mask));
        const int64_t blocks = std::min<int64_t>(nlines * ((npt + 256 / np - 1) / (256 / np)), 256 * 64);
#define ABZ_LO(NPV)                                                                                                           \
    {                                                                                                                         \
        ABZ_HIP(hipFuncSetAttribute((const void*)ltm_orb_rows_kernel<NPV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        launch(ctx, (ltm_orb_rows_kernel<NPV>), dim3((unsigned)blocks), dim3(256), lds, a);                                   \
    }
        if (np == 8) ABZ_LO(8)
        else if (np == 16) ABZ_LO(16)
        else ABZ_LO(32)
#undef ABZ_LO
    }
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

int ltm_projector_components(const int32_t* pairs, int npairs) {
    int ncomp = 0;
    for (int i = 0; i < npairs; ++i) ncomp += pairs[2 * i] == pairs[2 * i + 1] ? 1 : 2;
    return ncomp;
}

int launch_ltm_projectors(abz_ctx* ctx, int n, int npt, int64_t nlines, PlaneView H, PlaneView A, const int32_t* pairs, int npairs) {
    if (nlines <= 0) return ABZ_OK;
    LtmProjArgs a;
    a.H = H;
    a.A = A;
    a.nlines = nlines;
    a.n = n;
    a.npt = npt;
    a.npairs = npairs;
    a.ncomp = 0;
    for (int i = 0; i < ABZ_LTM_MAX_COMP; ++i) {
        a.p[i] = i < npairs ? pairs[2 * i] : 0;
        a.q[i] = i < npairs ? pairs[2 * i + 1] : 0;
        a.c0[i] = a.ncomp;
        if (i < npairs) a.ncomp += a.p[i] == a.q[i] ? 1 : 2;
    }
    ProfScope ps(ctx, ABZ_K_EIG);
    if (n <= 4) {
        const dim3 grid((unsigned)((nlines * A.row + 255) / 256));
        switch (n) {
            case 1: launch(ctx, ltm_proj_lane_kernel<1>, grid, dim3(256), 0, a); break;
            case 2: launch(ctx, ltm_proj_lane_kernel<2>, grid, dim3(256), 0, a); break;
            case 3: launch(ctx, ltm_proj_lane_kernel<3>, grid, dim3(256), 0, a); break;
            default: launch(ctx, ltm_proj_lane_kernel<4>, grid, dim3(256), 0, a); break;
        }
    } else {
        const int np = n <= 8 ? 8 : (n <= 16 ? 16 : 32);
        const size_t lds = ltm_orb_lds_bytes(np, a.ncomp);  // the tile holds every component
        const int64_t blocks = std::min<int64_t>(nlines * ((npt + 256 / np - 1) / (256 / np)), 256 * 64);
#define ABZ_LP(NPV)                                                                                                            \
    {                                                                                                                          \
        ABZ_HIP(hipFuncSetAttribute((const void*)ltm_proj_rows_kernel<NPV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
        launch(ctx, (ltm_proj_rows_kernel<NPV>), dim3((unsigned)blocks), dim3(256), lds, a);                                   \
    }
        if (np == 8) ABZ_LP(8)
        else if (np == 16) ABZ_LP(16)
        else ABZ_LP(32)
#undef ABZ_LP
    }
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
