// Fused GGR build for 5...32 bands (ref: src/dos_ggr.jl:14-44 -- `e, U = eigen(Hermitian(h))`, `v_j = Re diag(U' dH/dk_j U) t_j`,
// LAPACK there): ONE kernel per build, row layout (NP = 8 / 16 / 32 lanes per node), only (e, v) reach HBM.
//
// Per node, with lane r of its NP lanes owning row r of every matrix in registers:
//   (1) H(k) from the line's level-1 coefficient set staged in LDS (rows_device.h);
//   (2) Householder tridiagonalisation, the reflectors KEPT: lane r holds component r of every v_K, beta_K lives in lane
//       K + 1, the accumulated phase of the complex subdiagonal in the lane of its row (T_complex = P T_real P^H);
//   (3) eigenvalue b of the real tridiagonal in lane b: Sturm bisection + interpolation (tri_eigval_bisect);
//   (4) its eigenvector IN THE SAME LANE, no cross-lane traffic: inverse iteration on T - lambda_b I with the pivoted LU of
//       LAPACK's dlagtf / dlagts (dstein's scheme: three solves from a lane-dependent start vector, tiny pivots replaced by
//       eps ||T||); members of a cluster (chain of gaps <= 1e-5 ||T||: degenerate levels, where ANY orthonormal basis of the
//       eigenspace is an answer) are perturbed apart by 10 eps like dstein does and re-orthogonalised, lowest first, in
//       wave-uniform rounds that run only when a wave holds a cluster;
//   (5) back-transformation u_b = H_0 ... H_{n-3} P z_b: lane b owns COLUMN b of U.  The reflectors wait in LDS, in the room
//       of the coefficient set (idle between two series evaluations; packed lower triangle per node, written by the lanes
//       that own the components during the Householder steps) and come back by broadcast reads: kept in registers they
//       cost 2 NP doubles per lane beside the 4 NP of the tridiagonal LU -- 1.8 KB of scratch per lane at 16 bands;
//   (6) per direction j: the line's level-1 set of dH/dk_j is staged (variable 1: the same set with the factor 2 pi i f
//       applied on its way into LDS; variables 2, 3: families contracted with the factor on that variable), row r of it
//       evaluated in lane r, its upper triangle parked in the same LDS room, and v_b = u_b^H D u_b = sum_r D_rr |u_r|^2 +
//       2 Re sum_{r<c} conj(u_r) D_rc u_c from broadcast reads -- n^2 / 2 per direction, no matrix reaches HBM;
//   (7) e and v leave through an LDS tile [plane][node] as whole 128-B lines of the rule's planes.
// The round-4 route for these band counts wrote U and every dH/dk_j to HBM (4 KB per node and matrix at 16 bands), found
// the eigenvectors by n dense inverse iterations (n^4) and, above 16 bands, fell back to one wave per node:
// 24^3 nodes: 16 bands 1.54 ms, 17 bands 13.8 ms, 32 bands 29.5 ms.
#include <utility>

#include "abz_internal.h"
#include "rows_device.h"
#include "rows_eigvec.h"

namespace abz {

namespace {

constexpr double TWO_PI_R = 6.283185307179586476925286766559;

struct GgrRowsArgs {
    const double2* src[3];  // level-1 sets [line][M][n * n]: plain, derivative factor on variable 2, on variable 3
    const double2* tab;     // e^{2 pi i j / npt}
    PlaneView E, V;
    int64_t nlines;
    const int64_t* run_start;  // irregular lists: line l owns nodes [run_start[l], run_start[l + 1]) with grid indices gi
    const int32_t* gi;
    int n, M, first, npt, d;
    int mc;  // coefficients staged at a time (= M when the set fits the LDS whole)
    int fold;  // padded sets with a symmetric frequency range: staged folded (c_0, c_f +- c_f^T), half the series FMAs
    int coef_elems;  // complex numbers of the coefficient room (>= the staged chunk and >= the nodes' scratchpad rooms)
};

// (steps 2-5 -- kept reflectors, tridiagonal eigenvectors, back-transformation: rows_eigvec.h)

// (u^H D u from the node's LDS room -- park_upper, quad_form: rows_eigvec.h as well)

// stage coefficients [m0, m0 + mcur) of one level-1 set; DERIV: times 2 pi i (first + m) on the way (d/dk_1)
template <int NP, bool PAD>
__device__ __forceinline__ void ggr_stage(double2* coef, const double2* __restrict__ src, int n, int m0, int mcur, int first, bool deriv) {
    const int nn = n * n;
    if constexpr (PAD) {
        for (int t = threadIdx.x; t < mcur * NP * NP; t += blockDim.x) {
            const int m = t / (NP * NP), e = t - m * (NP * NP);
            const int rr = e % NP, j = e / NP;
            double2 c = (rr < n && j < n) ? src[(size_t)(m0 + m) * nn + rr + n * j] : make_double2(0.0, 0.0);
            if (deriv) {
                const double tf = TWO_PI_R * (double)(first + m0 + m);
                c = make_double2(-tf * c.y, tf * c.x);
            }
            coef[t] = c;
        }
    } else {
        for (int t = threadIdx.x; t < mcur * nn; t += blockDim.x) {
            double2 c = src[(size_t)m0 * nn + t];
            if (deriv) {
                const double tf = TWO_PI_R * (double)(first + m0 + t / nn);
                c = make_double2(-tf * c.y, tf * c.x);
            }
            coef[t] = c;
        }
    }
}

// the folded form of a set (panel_stage_fold of rows_device.h, here with the derivative factor of variable 1 and no shift):
// block 0 = -c_0 (zero for d/dk_1), block 2 f - 1 = s_f = c_f + c_f^T, block 2 f = t_f = c_f - c_f^T, c_f times 2 pi i f first
template <int NP>
__device__ __forceinline__ void ggr_stage_fold(double2* coef, const double2* __restrict__ src, int n, int M, bool deriv) {
    const int F = (M - 1) / 2, nn = n * n;
    for (int t = threadIdx.x; t < M * NP * NP; t += blockDim.x) {
        const int b = t / (NP * NP), e = t - b * (NP * NP);
        const int rr = e % NP, j = e / NP;
        double2 v = make_double2(0.0, 0.0);
        if (rr < n && j < n) {
            if (b == 0) {
                const double2 c = src[(size_t)F * nn + rr + n * j];
                v = deriv ? v : make_double2(-c.x, -c.y);
            } else {
                const int f = (b + 1) >> 1;
                double2 c = src[(size_t)(F + f) * nn + rr + n * j], cp = src[(size_t)(F + f) * nn + j + n * rr];
                if (deriv) {
                    const double tf = TWO_PI_R * (double)f;
                    c = make_double2(-tf * c.y, tf * c.x);
                    cp = make_double2(-tf * cp.y, tf * cp.x);
                }
                v = (b & 1) ? make_double2(c.x + cp.x, c.y + cp.y) : make_double2(c.x - cp.x, c.y - cp.y);
            }
        }
        coef[t] = v;
    }
}

template <int NP, bool PAD>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ggr_rows_kernel(GgrRowsArgs a) {
    extern __shared__ double2 lds_gr[];
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    const int n0 = a.n, nn = n0 * n0, M = a.M, mc = a.mc, d = a.d;
    double2* const coef = lds_gr;  // the staged coefficients; between two series evaluations: the nodes' rooms (PARK_STRIDE each)
    double* const tile = reinterpret_cast<double*>(coef + a.coef_elems);  // [(1 + d) NP][TS]
    const int slot = threadIdx.x / NP, r0 = threadIdx.x % NP, lane = threadIdx.x & 63;
    double2* const park = coef + (size_t)slot * PARK_STRIDE<NP>;
    int fm = a.first % a.npt;
    if (fm < 0) fm += a.npt;
    // work item = one pass (SLOTS nodes) of one line: the room of the coefficient set is reused between the series
    // evaluations, so every pass stages its sets anyway, and items of this size let the hardware's workgroup scheduler balance
    // a small grid (24^3 nodes, 16 bands: 576 lines = 1.1 rounds of workgroups when a workgroup took a whole line)
    const int ppl = (a.npt + SLOTS - 1) / SLOTS;  // passes per line (node lists: runs are at most npt long)
    for (int64_t item = blockIdx.x; item < a.nlines * ppl; item += gridDim.x) {
        const int64_t line = item / ppl;
        const int64_t kbase = a.run_start ? a.run_start[line] : line * a.npt;
        const int count = a.run_start ? (int)(a.run_start[line + 1] - kbase) : a.npt;
        const int i0 = (int)(item - line * ppl) * SLOTS;
        if (i0 < count) {  // (uniform)
            // n and r go through an opaque move once per pass: everything derived from them alone -- dozens of uniform
            // comparisons with n, the start vectors of the inverse iteration -- was hoisted out of both loops and lived (or
            // was spilled: 1.9 KB of scratch per lane) through the whole kernel
            int n = n0, r = r0;
            asm volatile("" : "+s"(n));
            asm volatile("" : "+v"(r));
            // a wave without a node in this pass computes nothing but keeps the block's barriers
            const bool wave_on = i0 + (int)(threadIdx.x >> 6) * (64 / NP) < count;
            const int i1 = i0 + slot;
            const bool act = i1 < count;
            const int ii = act ? i1 : 0;
            const int ic = a.gi ? a.gi[kbase + ii] : ii;
            const double2 z = a.tab[ic];
            const double2 w = a.tab[(int)(((unsigned)fm * (unsigned)ic) % (unsigned)a.npt)];
            double hr[NP], hi[NP];
            // row r of the series of family `fam` (deriv1: d/dk_1 of the plain family); every thread keeps the barriers
            auto series = [&](int fam, bool deriv1) {
                const double2* __restrict__ src = a.src[fam] + line * ((int64_t)M * nn);
                double pr = w.x, pi = w.y;
#pragma unroll
                for (int j = 0; j < NP; ++j) {
                    hr[j] = 0.0;
                    hi[j] = 0.0;
                }
                bool folded = false;
                if constexpr (PAD) {
                    if (a.fold) {  // (uniform) the whole set, folded: rows of -H from half the FMAs
                        folded = true;
                        __syncthreads();
                        ggr_stage_fold<NP>(coef, src, n, M, deriv1);
                        __syncthreads();
                        if (wave_on) panel_series_row_fold<NP>(coef, M, z.x, z.y, r, hr, hi);
                    }
                }
                for (int m0 = 0; m0 < M && !folded; m0 += mc) {
                    const int mcur = min(mc, M - m0);
                    __syncthreads();
                    ggr_stage<NP, PAD>(coef, src, n, m0, mcur, a.first, deriv1);
                    __syncthreads();
                    if (wave_on) {
                        if constexpr (PAD)  // (the padded set is always staged whole: one chunk)
                            panel_series_row<NP, true>(coef, n, mcur, z.x, z.y, pr, pi, r, hr, hi);
                        else
                            panel_series_row_chunk<NP>(coef, n, mcur, z.x, z.y, pr, pi, r, hr, hi);
                    }
                }
                __syncthreads();  // every wave is done with the set: its room serves as the nodes' scratchpad now
#pragma unroll
                for (int j = 0; j < NP; ++j) {  // the series routines accumulate -H; rows / columns >= n: zero
                    const bool real = r < n && j < n;
                    hr[j] = real ? -hr[j] : 0.0;
                    hi[j] = real ? -hi[j] : 0.0;
                }
            };
            series(0, false);
            double myeig = 0.0, ur[NP], ui[NP];
#pragma unroll
            for (int j = 0; j < NP; ++j) {
                ur[j] = 0.0;
                ui[j] = 0.0;
            }
            if (wave_on) rows_eigh_columns<NP>(n, r, lane, park, hr, hi, myeig, ur, ui);
            const bool keep = act && r < n;
            if (keep) tile[r * TS + slot] = myeig;
            for (int j = 0; j < d; ++j) {
                series(j, j == 0);
                if (wave_on) {
                    park_upper<NP>(n, r, park, hr, hi);
                    wave_sync_lds();
                    const double v = quad_form<NP>(n, park, ur, ui, std::make_integer_sequence<int, NP>());
                    if (keep) tile[((1 + j) * NP + r) * TS + slot] = v;
                }
            }
            __syncthreads();
            const int nplanes = (1 + d) * n;
            for (int idx = threadIdx.x; idx < nplanes * SLOTS; idx += 256) {
                const int pl = idx / SLOTS, sl = idx - pl * SLOTS;
                if (i0 + sl >= count) continue;
                const int64_t k = kbase + i0 + sl;
                if (pl < n) {
                    a.E.base[view_off(a.E, k) + (int64_t)pl * a.E.pitch] = tile[pl * TS + sl];
                } else {
                    const int q = pl - n, j = q / n, b = q - j * n;
                    a.V.base[view_off(a.V, k) + (int64_t)(j * n + b) * a.V.pitch] = tile[((1 + j) * NP + b) * TS + sl];
                }
            }
            // (the next pass begins with a barrier before it touches the LDS again)
        }
    }
}

size_t ggr_rows_tile_bytes(int np, int d) { return sizeof(double) * (size_t)((1 + d) * np) * (size_t)(256 / np + 1); }
// the nodes' scratchpad rooms of one workgroup (complex numbers)
size_t ggr_rows_park_elems(int np) { return (size_t)(256 / np) * (size_t)(np * (np + 1) / 2 + 1); }

}  // namespace

// Hermitian series of 5...32 bands, full grids or node lists that come in runs per level-1 set (d >= 2)
bool ggr_rows_supported(int n, int d, int M, int npt, bool herm) {
    if (!herm || n <= 4 || n > 32 || d < 1 || d > 3 || npt < 1 || npt >= 65536 || M < 1) return false;
    const int np = n <= 8 ? 8 : (n <= 16 ? 16 : 32);
    // one coefficient at a time always fits beside the rooms' minimum
    return sizeof(double2) * std::max((size_t)n * n, ggr_rows_park_elems(np)) + ggr_rows_tile_bytes(np, d) <= 150 * 1024;
}

int launch_ggr_rows(abz_ctx* ctx, const GgrRowsSpec& gs) {
    if (gs.nlines <= 0) return ABZ_OK;
    GgrRowsArgs a;
    for (int j = 0; j < 3; ++j) a.src[j] = gs.src[j];
    a.tab = gs.tab;
    a.E = gs.E;
    a.V = gs.V;
    a.nlines = gs.nlines;
    a.run_start = gs.run_start;
    a.gi = gs.gi;
    a.n = gs.n;
    a.M = gs.M;
    a.first = gs.first;
    a.npt = gs.npt;
    a.d = gs.d;
    const int np = gs.n <= 8 ? 8 : (gs.n <= 16 ? 16 : 32);
    const size_t tile = ggr_rows_tile_bytes(np, gs.d), park = ggr_rows_park_elems(np);
    // the zero-padded set whole when two workgroups per CU still fit (<= 72 KB each); otherwise unpadded, as many coefficients
    // at a time as fit (whole up to 150 KB)
    const bool pad = sizeof(double2) * std::max((size_t)gs.M * np * np, park) + tile <= 72 * 1024;
    size_t elems;
    if (pad) {
        a.mc = gs.M;
        elems = (size_t)gs.M * np * np;
    } else {
        const size_t per = (size_t)gs.n * gs.n;
        if (sizeof(double2) * std::max(per * (size_t)gs.M, park) + tile <= 150 * 1024) {
            a.mc = gs.M;
        } else {
            a.mc = (int)((72 * 1024 - tile) / (sizeof(double2) * per));
            if (a.mc < 1) a.mc = (int)((150 * 1024 - tile) / (sizeof(double2) * per));
            if (a.mc < 1) {
                set_error("GGR build: one %d-band coefficient block does not fit the LDS", gs.n);
                return ABZ_ERR_UNSUPPORTED;
            }
        }
        elems = per * (size_t)a.mc;
    }
    a.fold = (pad && (gs.M & 1) && gs.first == -((gs.M - 1) / 2) && abz_switch(SW_EIG_FOLD) != 0) ? 1 : 0;
    elems = std::max(elems, park);
    a.coef_elems = (int)elems;
    const size_t lds = sizeof(double2) * elems + tile;
    const int64_t blocks = std::min<int64_t>(gs.nlines * ((gs.npt + 256 / np - 1) / (256 / np)), 256 * 64);
    ProfScope ps(ctx, ABZ_K_EVAL);
#define ABZ_GR(NPV, PV)                                                                                                              \
    {                                                                                                                                \
        ABZ_HIP(hipFuncSetAttribute((const void*)ggr_rows_kernel<NPV, PV>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));   \
        launch(ctx, (ggr_rows_kernel<NPV, PV>), dim3((unsigned)blocks), dim3(256), lds, a);                      \
    }
    if (np == 8 && pad) ABZ_GR(8, true)
    else if (np == 8) ABZ_GR(8, false)
    else if (np == 16 && pad) ABZ_GR(16, true)
    else if (np == 16) ABZ_GR(16, false)
    else if (pad) ABZ_GR(32, true)
    else ABZ_GR(32, false)
#undef ABZ_GR
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
