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
// The band projectors U_pb conj(U_qb) of abz_rule_ltm_projectors are the second half of the file.  Loads, pass head, write-out
// and launch are the frame of ltm_eig_device.h (the two row kernels keep the row load written out: see herm_row_load).
#include "ltm_eig_device.h"

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

template <int N>
__global__ __launch_bounds__(256) void ltm_orb_lane_kernel(LtmOrbArgs a) {
    const int row = a.A.row;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t / row;
    const int i = (int)(t - line * row);
    double w[N][N];  // [band][orbital]
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int o = 0; o < N; ++o) w[b][o] = 0.0;
    }
    if (i < a.npt) {
        if constexpr (N == 1) {
            w[0][0] = 1.0;
        } else {
            CMat<N> h, V;
            herm_lane_load<N>(a.H, line, i, h);
            double e[N];
            herm_eig<N, true>(h, e, V);
#pragma unroll
            for (int b = 0; b < N; ++b) {
#pragma unroll
                for (int o = 0; o < N; ++o) w[b][o] = proj_diag(V.re[o][b], V.im[o][b]);
            }
        }
    }
    double* __restrict__ const out = a.A.base + line * a.A.tile + i;
    for (int c = 0; c < a.ncomp; ++c) {
        const int o = a.orb[c];  // (uniform)
#pragma unroll
        for (int b = 0; b < N; ++b) out[(int64_t)(c * N + b) * a.A.pitch] = xp_pick(w[b], o);
    }
}

template <int NP>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ltm_orb_rows_kernel(LtmOrbArgs a) {
    extern __shared__ double2 lds_orb[];
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    double* const tile = reinterpret_cast<double*>(lds_orb + SLOTS * PARK_STRIDE<NP>);  // [asked orbital][NP bands][TS]
    const int npt = a.npt, nplanes = a.ncomp * a.n;
    for (int64_t item = blockIdx.x; item < a.nlines * rows_passes_per_line<NP>(npt); item += gridDim.x) {
        const RowsPass<NP> ps = rows_pass<NP>(lds_orb, item, npt, a.n);
        const int n = ps.n, r = ps.r;
        if (ps.wave_on) {
            double hr[NP], hi[NP];
            // herm_row_load written out (see there: behind the call this kernel's solve gets other arithmetic at NP = 16)
            const double* __restrict__ const in = a.H.base + ps.line * a.H.tile + (ps.act ? ps.i1 : 0);
            const int rr = r < n ? r : n - 1;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                hr[j] = 0.0;
                hi[j] = 0.0;
                if (j < n) {  // uniform
                    const int lo = rr < j ? rr : j, up = rr < j ? j : rr;
                    const int64_t pl = herm_plane(a.H, n, lo, up);
                    const double re = in[pl * a.H.pitch];
                    const double im = in[(pl + (lo != up ? 1 : 0)) * a.H.pitch];
                    hr[j] = r < n ? re : 0.0;
                    hi[j] = (r < n && lo != up) ? (rr < j ? im : -im) : 0.0;
                }
            }
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, ps.lane, ps.park, hr, hi, myeig, ur, ui);
            if (ps.act && r < n) {
                int rank = 0;  // position of orbital o among the asked ones
#pragma unroll
                for (int o = 0; o < NP; ++o) {
                    if (o < n && ((a.mask >> o) & 1u)) {  // uniform
                        tile[(rank * NP + r) * TS + ps.slot] = proj_diag(ur[o], ui[o]);
                        ++rank;
                    }
                }
            }
        }
        __syncthreads();
        rows_tile_write<NP>(a.A, ps.line, ps.i0, npt, n, nplanes, tile,
                            [&](int c, int b) { return __popc(a.mask & ((1u << a.orb[c]) - 1u)) * NP + b; });
        __syncthreads();  // the tile is free for the next pass
    }
}

// ---- band projectors P^b_pq(k) = U_pb conj(U_qb) (abz_rule_ltm_projectors) ---------------------------------------------------
// The two kernels above with another product formed from column b of U.  Pair i = (p[i], q[i]) fills components c0[i]
// (p == q: |U_pb|^2, the expression of the orbital weights, bit for bit) or c0[i], c0[i] + 1 (p != q: Re and Im of the
// projector).  The phase of an eigenvector cancels in the product, so no gauge is fixed anywhere.  p and q are uniform but
// known at run time only: the values are picked by select chains (xp_pick: an index into a register array would be scratch).
struct LtmProjArgs {
    PlaneView H, A;
    int64_t nlines;
    int n, npt, npairs, ncomp;
    int p[ABZ_LTM_MAX_COMP], q[ABZ_LTM_MAX_COMP], c0[ABZ_LTM_MAX_COMP];
};

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
            CMat<N> h, V;
            herm_lane_load<N>(a.H, line, i, h);
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
            const double pr = xp_pick(ur[b], p), pi = xp_pick(ui[b], p);
            if (p == q) {
                out[(int64_t)(c * N + b) * a.A.pitch] = proj_diag(pr, pi);
            } else {
                const double qr = xp_pick(ur[b], q), qi = xp_pick(ui[b], q);
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
    double* const tile = reinterpret_cast<double*>(lds_orb + SLOTS * PARK_STRIDE<NP>);  // [component][NP bands][TS]
    const int npt = a.npt, nplanes = a.ncomp * a.n;
    for (int64_t item = blockIdx.x; item < a.nlines * rows_passes_per_line<NP>(npt); item += gridDim.x) {
        const RowsPass<NP> ps = rows_pass<NP>(lds_orb, item, npt, a.n);
        const int n = ps.n, r = ps.r;
        if (ps.wave_on) {
            double hr[NP], hi[NP];
            // herm_row_load written out (see there: behind the call this kernel's results move in the last bit at NP = 32)
            const double* __restrict__ const in = a.H.base + ps.line * a.H.tile + (ps.act ? ps.i1 : 0);
            const int rr = r < n ? r : n - 1;
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                hr[j] = 0.0;
                hi[j] = 0.0;
                if (j < n) {  // uniform
                    const int lo = rr < j ? rr : j, up = rr < j ? j : rr;
                    const int64_t pl = herm_plane(a.H, n, lo, up);
                    const double re = in[pl * a.H.pitch];
                    const double im = in[(pl + (lo != up ? 1 : 0)) * a.H.pitch];
                    hr[j] = r < n ? re : 0.0;
                    hi[j] = (r < n && lo != up) ? (rr < j ? im : -im) : 0.0;
                }
            }
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, ps.lane, ps.park, hr, hi, myeig, ur, ui);
            if (ps.act && r < n) {
                for (int k = 0; k < a.npairs; ++k) {
                    const int p = a.p[k], q = a.q[k], c = a.c0[k];  // (uniform)
                    const double pr = xp_pick(ur, p), pi = xp_pick(ui, p);
                    if (p == q) {
                        tile[(c * NP + r) * TS + ps.slot] = proj_diag(pr, pi);
                    } else {
                        const double qr = xp_pick(ur, q), qi = xp_pick(ui, q);
                        tile[(c * NP + r) * TS + ps.slot] = proj_re(pr, pi, qr, qi);
                        tile[((c + 1) * NP + r) * TS + ps.slot] = proj_im(pr, pi, qr, qi);
                    }
                }
            }
        }
        __syncthreads();
        rows_tile_write<NP>(a.A, ps.line, ps.i0, npt, n, nplanes, tile, [](int c, int b) { return c * NP + b; });
        __syncthreads();  // the tile is free for the next pass
    }
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
    int rc;
    if (n <= 4) {
        rc = lanes_dispatch(n, [&](auto N) { return launch_lanes(ctx, ltm_orb_lane_kernel<decltype(N)::value>, nlines, A.row, a); });
    } else {
        const int np = rows_np(n);
        const size_t lds = rows_lds_bytes(np, rows_tile_bytes(np, __builtin_popcount(a.mask)));
        const dim3 grid((unsigned)rows_blocks(np, npt, nlines, 256 * 64));
        rc = rows_dispatch(np, [&](auto NP) { return launch_rows(ctx, ltm_orb_rows_kernel<decltype(NP)::value>, grid, lds, a); });
    }
    if (rc) return rc;
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
    int rc;
    if (n <= 4) {
        rc = lanes_dispatch(n, [&](auto N) { return launch_lanes(ctx, ltm_proj_lane_kernel<decltype(N)::value>, nlines, A.row, a); });
    } else {
        const int np = rows_np(n);
        const size_t lds = rows_lds_bytes(np, rows_tile_bytes(np, a.ncomp));  // the tile holds every component
        const dim3 grid((unsigned)rows_blocks(np, npt, nlines, 256 * 64));
        rc = rows_dispatch(np, [&](auto NP) { return launch_rows(ctx, ltm_proj_rows_kernel<decltype(NP)::value>, grid, lds, a); });
    }
    if (rc) return rc;
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
