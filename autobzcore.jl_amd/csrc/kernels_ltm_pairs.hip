// Pair rules of the tetrahedron method (abz_rule_ltm_pairs): for a lower range [v0, v0 + nv) and an upper range [c0, c0 + nc) of the
// ascending bands of a whole periodic grid, pseudo-band p = (v - v0) nc + (c - c0),
//   ltm_pair_energy_kernel   Delta_p = e_c - e_v from the eigenvalue planes of the source rule, one subtraction, padding columns 0.0;
//   the element kernels      M^i_vc = u_v(k)^H Hermitian(O_i(k)) u_c(k) for up to ABZ_LTM_PAIRS_MAX_OPS operator rules of the same grid,
//                            component c = Re or Im of M^i_vc conj(M^j_vc) -- no phase of u_v or u_c changes it -- into the element
//                            block of abz_rule_ltm_elements (plane c nb + p of a grid line's tile, padded rows, padding columns 0.0).
// The element kernels read H and O (upper triangles, either plane layout, each rule with its own tiling) through the frame of
// ltm_eig_device.h, which also has their pass head and their launch; neither U nor O u reaches HBM, no atomics, no dependence
// on the launch geometry: two calls write the same bits.
//   2...4 bands   one grid point per lane: herm_eig<N, true>, then per operator y_c = O u_c and M_vc = u_v^H y_c for the
//                 N (N - 1) / 2 pairs v < c in registers (all indices compile-time; the pairs outside the ranges are computed and
//                 not stored); the products are formed at the store.
//   5...32 bands  NP = 8 / 16 / 32 lanes per node: after rows_eigh_columns (column b of U in lane b) lane r loads row r of O_i and
//                 parks its upper triangle in the node's LDS room (park_upper, as the expectation kernel does), and EVERY lane forms
//                 the full Hermitian mat-vec y_b = O_i u_b from broadcast reads of the room (herm_matvec).  Then the columns of the
//                 smaller side are parked in the same room -- u_v of the lower range if nv <= nc, else y_c of the upper range;
//                 min(nv, nc) n <= n^2 / 2 complex numbers fit the n (n + 1) / 2 + 1 of PARK_STRIDE -- and the lanes of the other
//                 side form their min(nv, nc) dot products from broadcast reads: no cross-lane shuffles.  The complex M^i_vc leave
//                 the lanes into an LDS tile [operator][pair][node]; Re / Im (M^i conj M^j) are formed during the write-out of
//                 contiguous row segments, so no lane keeps nv nops complex values alive and no register array is indexed at run
//                 time (xp_pick, xp_put).
// LDS per workgroup: the rooms (18.5 / 34.3 / 66.1 KB at NP = 8 / 16 / 32) plus 16 B nops npairs (256 / NP + 1) for the tile, sized by
// the call: at most 33 KB (NP = 8, 4 x 4 pairs), 68 KB (NP = 16, 64 pairs) and 36 KB (NP = 32, 64 pairs) with 4 operators.  NP = 16
// with 4 operators and 64 pairs is one workgroup per CU (102 KB of 160); up to 2 operators, or up to 32 pairs, leave room for two.
// At a degenerate level u_v, u_c are some orthonormal bases of their eigenspaces: only the sum of a component over all pairs
// between two levels is defined.
#include "ltm_eig_device.h"

namespace abz {

namespace {

constexpr int POPS = ABZ_LTM_PAIRS_MAX_OPS;

struct LtmPairsArgs {
    PlaneView H;        // H planes of the grid (full or Hermitian-compact)
    PlaneView O[POPS];  // the operators' planes, each in its own layout and tiling
    PlaneView A;        // the element block: ncomp nv nc planes, tiled like the eigenvalue planes of the pair rule
    int64_t nlines;
    int n, npt, nops, ncomp;
    int v0, nv, c0, nc;
    int ci[ABZ_LTM_MAX_COMP], cj[ABZ_LTM_MAX_COMP], part[ABZ_LTM_MAX_COMP];  // component c: Re (part 0) / Im (1) of M^ci conj(M^cj)
};

// Re or Im of a conj(b).  The imaginary part from two rounded products, not a fused one: Im |M|^2 is then exactly zero, and
// Im M^i conj(M^j) = -Im M^j conj(M^i) to the bit (the products go through an opaque move: the compiler contracts a
// multiplication and a subtraction into an fma wherever it sees them together, __dmul_rn included)
__device__ __forceinline__ double pair_product(double ar, double ai, double br, double bi, int part) {
    double p = ai * br, q = ar * bi;
    asm volatile("" : "+v"(p), "+v"(q));
    return part ? p - q : fma(ar, br, ai * bi);
}

__global__ __launch_bounds__(256) void ltm_pair_energy_kernel(PlaneView E, PlaneView D, int64_t nlines, int npt, int v0, int nv, int c0, int nc) {
    const int row = D.row;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nlines * row) return;
    const int64_t line = t / row;
    const int i = (int)(t - line * row);
    const bool node = i < npt;  // (the source's planes are read at its nodes only: its padding may hold anything)
    const double* __restrict__ const in = E.base + line * E.tile + (node ? i : 0);
    double* __restrict__ const out = D.base + line * D.tile + i;
    // nv + nc loads per node: the smaller range (at most 8 bands, nv nc <= 64) waits in registers, all indices compile-time
    const bool lowreg = nv <= nc;
    const int cnt = lowreg ? nv : nc, first = lowreg ? v0 : c0;
    double held[8];
#pragma unroll
    for (int m = 0; m < 8; ++m) held[m] = m < cnt ? in[(int64_t)(first + m) * E.pitch] : 0.0;
    if (lowreg) {
        for (int c = 0; c < nc; ++c) {
            const double ec = in[(int64_t)(c0 + c) * E.pitch];
#pragma unroll
            for (int m = 0; m < 8; ++m)
                if (m < nv) out[(int64_t)(m * nc + c) * D.pitch] = node ? ec - held[m] : 0.0;
        }
    } else {
        for (int v = 0; v < nv; ++v) {
            const double ev = in[(int64_t)(v0 + v) * E.pitch];
#pragma unroll
            for (int m = 0; m < 8; ++m)
                if (m < nc) out[(int64_t)(v * nc + m) * D.pitch] = node ? held[m] - ev : 0.0;
        }
    }
}

template <int N>
__global__ __launch_bounds__(256) void ltm_pairs_lane_kernel(LtmPairsArgs a) {
    constexpr int NPAIR = N * (N - 1) / 2;  // (v, c), v < c, at c (c - 1) / 2 + v
    const int row = a.A.row;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t / row;
    const int i = (int)(t - line * row);
    double mr[NPAIR][POPS], mi[NPAIR][POPS];  // [pair][operator]; zeros in the padding columns
#pragma unroll
    for (int p = 0; p < NPAIR; ++p) {
#pragma unroll
        for (int k = 0; k < POPS; ++k) {
            mr[p][k] = 0.0;
            mi[p][k] = 0.0;
        }
    }
    if (i < a.npt) {
        CMat<N> V;
        {
            CMat<N> h;
            herm_lane_load<N>(a.H, line, i, h);
            double e[N];
            herm_eig<N, true>(h, e, V);
        }
        for (int k = 0; k < a.nops; ++k) {  // (uniform)
            const PlaneView& O = a.O[k];
            const double* __restrict__ const in = O.base + line * O.tile + i;
            double yr[N][N], yi[N][N];  // y[p][c] = (O u_c)_p
#pragma unroll
            for (int p = 0; p < N; ++p) {
#pragma unroll
                for (int c = 0; c < N; ++c) {
                    yr[p][c] = 0.0;
                    yi[p][c] = 0.0;
                }
            }
#pragma unroll
            for (int s = 0; s < N; ++s) {
#pragma unroll
                for (int p = 0; p <= s; ++p) {
                    const int64_t pl = herm_plane(O, N, p, s);
                    const double ore = in[pl * O.pitch];
                    if (p == s) {
#pragma unroll
                        for (int c = 0; c < N; ++c) {
                            yr[p][c] = fma(ore, V.re[p][c], yr[p][c]);
                            yi[p][c] = fma(ore, V.im[p][c], yi[p][c]);
                        }
                    } else {
                        const double oim = in[(pl + 1) * O.pitch];
#pragma unroll
                        for (int c = 0; c < N; ++c) {
                            // y_p += O_ps u_s,  y_s += conj(O_ps) u_p
                            yr[p][c] = fma(ore, V.re[s][c], fma(-oim, V.im[s][c], yr[p][c]));
                            yi[p][c] = fma(ore, V.im[s][c], fma(oim, V.re[s][c], yi[p][c]));
                            yr[s][c] = fma(ore, V.re[p][c], fma(oim, V.im[p][c], yr[s][c]));
                            yi[s][c] = fma(ore, V.im[p][c], fma(-oim, V.re[p][c], yi[s][c]));
                        }
                    }
                }
            }
#pragma unroll
            for (int c = 1; c < N; ++c) {
#pragma unroll
                for (int v = 0; v < c; ++v) {
                    double sr = 0.0, si = 0.0;  // conj(u_v) . y_c
#pragma unroll
                    for (int p = 0; p < N; ++p) {
                        sr = fma(V.re[p][v], yr[p][c], fma(V.im[p][v], yi[p][c], sr));
                        si = fma(V.re[p][v], yi[p][c], fma(-V.im[p][v], yr[p][c], si));
                    }
                    xp_put(mr[c * (c - 1) / 2 + v], k, sr);
                    xp_put(mi[c * (c - 1) / 2 + v], k, si);
                }
            }
        }
    }
    double* __restrict__ const out = a.A.base + line * a.A.tile + i;
    const int nb = a.nv * a.nc;
    for (int cc = 0; cc < a.ncomp; ++cc) {
        const int ki = a.ci[cc], kj = a.cj[cc], part = a.part[cc];  // (uniform)
#pragma unroll
        for (int c = 1; c < N; ++c) {
#pragma unroll
            for (int v = 0; v < c; ++v) {
                if (v >= a.v0 && v < a.v0 + a.nv && c >= a.c0 && c < a.c0 + a.nc) {  // uniform
                    const int pp = c * (c - 1) / 2 + v;
                    const double x = pair_product(xp_pick(mr[pp], ki), xp_pick(mi[pp], ki), xp_pick(mr[pp], kj), xp_pick(mi[pp], kj), part);
                    out[(int64_t)(cc * nb + (v - a.v0) * a.nc + (c - a.c0)) * a.A.pitch] = x;
                }
            }
        }
    }
}

// y = D u for this lane's column u, D Hermitian with its upper triangle parked in the node's room (park_upper): column C of the
// triangle at a time, D[R][C] feeds y_R with u_C and, conjugated, y_C with u_R (broadcast reads)
template <int NP, int C, int... RR>
__device__ __forceinline__ void matvec_col(int n, const double2* __restrict__ park, const double (&ur)[NP], const double (&ui)[NP], double (&yr)[NP],
                                           double (&yi)[NP], std::integer_sequence<int, RR...>) {
    if (C >= n) return;  // uniform
    const double2* __restrict__ col = park + C * (C + 1) / 2;
    const double ucr = ur[C], uci = ui[C];
    const double d = col[C].x;
    double cr = d * ucr, ci = d * uci;
    ((void)([&] {
         constexpr int R = RR;  // R < C
         const double2 dv = col[R];
         yr[R] = fma(dv.x, ucr, fma(-dv.y, uci, yr[R]));
         yi[R] = fma(dv.x, uci, fma(dv.y, ucr, yi[R]));
         cr = fma(dv.x, ur[R], fma(dv.y, ui[R], cr));
         ci = fma(dv.x, ui[R], fma(-dv.y, ur[R], ci));
     }()),
     ...);
    yr[C] += cr;
    yi[C] += ci;
}
template <int NP, int... CC>
__device__ __forceinline__ void herm_matvec(int n, const double2* __restrict__ park, const double (&ur)[NP], const double (&ui)[NP], double (&yr)[NP],
                                            double (&yi)[NP], std::integer_sequence<int, CC...>) {
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        yr[j] = 0.0;
        yi[j] = 0.0;
    }
    (matvec_col<NP, CC>(n, park, ur, ui, yr, yi, std::make_integer_sequence<int, CC>()), ...);
}

// sum_j conj(col[j]) x_j over the n entries of a parked column (broadcast reads)
template <int NP>
__device__ __forceinline__ void parked_dot(int n, const double2* __restrict__ col, const double (&xr)[NP], const double (&xi)[NP], double& sr, double& si) {
    double ar[2] = {0.0, 0.0}, ai[2] = {0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        if (j < n) {  // uniform
            const double2 a = col[j];
            ar[j & 1] = fma(a.x, xr[j], fma(a.y, xi[j], ar[j & 1]));
            ai[j & 1] = fma(a.x, xi[j], fma(-a.y, xr[j], ai[j & 1]));
        }
    }
    sr = ar[0] + ar[1];
    si = ai[0] + ai[1];
}

template <int NP>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ltm_pairs_rows_kernel(LtmPairsArgs a) {
    extern __shared__ double2 lds_pr[];
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    double2* const tile = lds_pr + SLOTS * PARK_STRIDE<NP>;  // [operator][pair][TS]
    const int npt = a.npt, nb = a.nv * a.nc;
    const bool lowpark = a.nv <= a.nc;  // the lower range's u_v are parked (else the upper range's y_c)
    for (int64_t item = blockIdx.x; item < a.nlines * rows_passes_per_line<NP>(npt); item += gridDim.x) {
        const RowsPass<NP> ps = rows_pass<NP>(lds_pr, item, npt, a.n);
        const int n = ps.n, r = ps.r, i0 = ps.i0;
        double2* const park = ps.park;  // this node's reflectors, then its operator, then the parked columns
        if (ps.wave_on) {
            const int column = ps.act ? ps.i1 : 0;
            double hr[NP], hi[NP];
            // (a local closure over the shared load, as these kernels had one over their own: with the direct calls the
            // NP = 16 kernel spills 624 B instead of 520)
            auto load_row = [&](const PlaneView& X) { herm_row_load<NP>(X, n, r, ps.line, column, hr, hi); };
            load_row(a.H);
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, ps.lane, park, hr, hi, myeig, ur, ui);
            const bool in_v = r >= a.v0 && r < a.v0 + a.nv, in_c = r >= a.c0 && r < a.c0 + a.nc;
            for (int k = 0; k < a.nops; ++k) {  // (uniform)
                load_row(a.O[k]);
                wave_sync_lds();  // every lane of the node is done reading the room (reflectors, the columns parked before)
                park_upper<NP>(n, r, park, hr, hi);
                wave_sync_lds();
                herm_matvec<NP>(n, park, ur, ui, hr, hi, std::make_integer_sequence<int, NP>());  // y_r = O_k u_r in the row registers
                wave_sync_lds();  // the operator has been read
                if (lowpark ? in_v : in_c) {
                    double2* const mine = park + (lowpark ? r - a.v0 : r - a.c0) * n;
#pragma unroll
                    for (int j = 0; j < NP; ++j)
                        if (j < n) mine[j] = lowpark ? make_double2(ur[j], ui[j]) : make_double2(hr[j], hi[j]);
                }
                wave_sync_lds();
                double2* const trow = tile + (size_t)k * nb * TS + ps.slot;
                if (lowpark) {  // lane c: M_vc = conj(u_v) . y_c over the parked u_v
                    for (int m = 0; m < a.nv; ++m) {
                        double sr, si;
                        parked_dot<NP>(n, park + m * n, hr, hi, sr, si);
                        if (ps.act && in_c) trow[(m * a.nc + (r - a.c0)) * TS] = make_double2(sr, si);
                    }
                } else {  // lane v: conj(M_vc) = conj(y_c) . u_v over the parked y_c
                    for (int m = 0; m < a.nc; ++m) {
                        double sr, si;
                        parked_dot<NP>(n, park + m * n, ur, ui, sr, si);
                        if (ps.act && in_v) trow[((r - a.v0) * a.nc + m) * TS] = make_double2(sr, -si);
                    }
                }
            }
        }
        __syncthreads();
        // the pass's columns of every plane; the line's last pass takes the padding columns along, as zeros
        const int width = (i0 + SLOTS >= npt) ? a.A.row - i0 : SLOTS;
        double* __restrict__ const out = a.A.base + ps.line * a.A.tile + i0;
        for (int cc = 0; cc < a.ncomp; ++cc) {
            const int part = a.part[cc];  // (uniform)
            const double2* __restrict__ const ti = tile + (size_t)a.ci[cc] * nb * TS;
            const double2* __restrict__ const tj = tile + (size_t)a.cj[cc] * nb * TS;
            for (int idx = threadIdx.x; idx < nb * width; idx += 256) {
                const int p = idx / width, sl = idx - p * width;
                double x = 0.0;
                if (i0 + sl < npt) {
                    const double2 mi = ti[p * TS + sl], mj = tj[p * TS + sl];
                    x = pair_product(mi.x, mi.y, mj.x, mj.y, part);
                }
                out[(int64_t)(cc * nb + p) * a.A.pitch + sl] = x;
            }
        }
        __syncthreads();  // the tile is free for the next pass
    }
}

}  // namespace

int launch_ltm_pair_energies(abz_ctx* ctx, int npt, int64_t nlines, PlaneView E, PlaneView D, int v0, int nv, int c0, int nc) {
    if (nlines <= 0) return ABZ_OK;
    ProfScope ps(ctx, ABZ_K_LTM);
    const dim3 grid((unsigned)((nlines * D.row + 255) / 256));
    launch(ctx, ltm_pair_energy_kernel, grid, dim3(256), 0, E, D, nlines, npt, v0, nv, c0, nc);
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

int launch_ltm_pairs(abz_ctx* ctx, int n, int npt, int64_t nlines, PlaneView H, const PlaneView* ops, int nops, PlaneView A, int v0, int nv,
                     int c0, int nc, const int32_t* comps, int ncomp) {
    if (nlines <= 0) return ABZ_OK;
    if (n < 2 || n > 32 || nops < 1 || nops > POPS || ncomp < 1 || ncomp > ABZ_LTM_MAX_COMP || v0 < 0 || nv < 1 || nc < 1 || v0 + nv > c0 ||
        c0 + nc > n) {
        set_error("launch_ltm_pairs: n = %d, nops = %d, ncomp = %d, ranges [%d, %d) x [%d, %d) out of range", n, nops, ncomp, v0, v0 + nv, c0,
                  c0 + nc);
        return ABZ_ERR_INTERNAL;
    }
    LtmPairsArgs a;
    a.H = H;
    a.A = A;
    a.nlines = nlines;
    a.n = n;
    a.npt = npt;
    a.nops = nops;
    a.ncomp = ncomp;
    a.v0 = v0;
    a.nv = nv;
    a.c0 = c0;
    a.nc = nc;
    for (int k = 0; k < POPS; ++k) a.O[k] = ops[k < nops ? k : 0];
    for (int c = 0; c < ABZ_LTM_MAX_COMP; ++c) {
        a.ci[c] = c < ncomp ? comps[3 * c] : 0;
        a.cj[c] = c < ncomp ? comps[3 * c + 1] : 0;
        a.part[c] = c < ncomp ? comps[3 * c + 2] : 0;
    }
    ProfScope ps(ctx, ABZ_K_EIG);
    int rc;
    if (n <= 4) {
        rc = lanes_dispatch(n, [&](auto N) {
            if constexpr (decltype(N)::value >= 2) return launch_lanes(ctx, ltm_pairs_lane_kernel<decltype(N)::value>, nlines, A.row, a);
            return (int)ABZ_ERR_INTERNAL;  // (n >= 2 was checked)
        });
    } else {
        const int np = rows_np(n);
        const size_t lds = rows_lds_bytes(np, sizeof(double2) * (size_t)nops * nv * nc * (256 / np + 1));  // the tile: complex M^i_vc
        const dim3 grid((unsigned)rows_blocks(np, npt, nlines, 256 * 64));
        rc = rows_dispatch(np, [&](auto NP) { return launch_rows(ctx, ltm_pairs_rows_kernel<decltype(NP)::value>, grid, lds, a); });
    }
    if (rc) return rc;
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
