// Density matrix of the tetrahedron method in the orbital basis (abz_rule_ltm_density_matrix):
//      rho_pq(E_i) = sum_k sum_b w_b(k; E_i) U_pb(k) conj(U_qb(k))
// from the resident integration weights of abz_rule_ltm_node_weights (plane i n + b of a grid line's tile: band b at E[i], padding
// columns zero) and the H planes of the same whole grid, in ONE eigen-solve per node (and group of energies): neither U nor the
// band projectors reach HBM.  The weights say what rho is: occupations, corrected occupations or the spectral-density matrix.
// U(k), the H layouts and the treatment of degenerate levels are those of kernels_ltm_orb.hip (lane load, pass head, products and
// launch: the frame of ltm_eig_device.h): a degenerate level gets some orthonormal basis, and only sums over a level with
// equal weights are defined.  The corrected weights do go negative: nothing here assumes w >= 0.
//   1...4 bands   ltm_dens_lane_kernel<N, NE>: one grid point per lane over a fixed grid-stride, herm_eig<N, true>, the weights of
//                 the launch's NE = 1 or 4 energies from the resident block, the upper triangle of sum_b w_b u_b u_b^dagger in
//                 registers as N^2 reals per energy (N diagonal entries, then Re and Im of every p < q, p outer), in the
//                 expressions of the projector kernels: a diagonal entry is sum_b w_b fma(re, re, im im).  Butterfly over the
//                 wave, the four waves in order through LDS.
//   5...32 bands  ltm_dens_rows_kernel<NP>, NP = 8 / 16 / 32 lanes per node, blockIdx.y = energy (the solve is repeated per
//                 energy: LDS holds one accumulator set).  rows_eigh_columns leaves column b of U in lane b; the contraction
//                 needs rows.  The node's reflector room `park` is dead after the solve and holds half of U: U goes through
//                 it once, in two halves of the orbital index (the upper one first), row stride NP + 1
//                 (NP/2 (NP + 1) <= PARK_STRIDE<NP>); the lanes of a half take their own row, scaled by the w_b of the node
//                 (NP doubles in LDS), into registers, and every lane q adds
//                      rho_pq += sum_b U_pb conj(w_b U_qb),   p <= q, p in the half,
//                 from broadcast reads of row p into the entry q (q + 1) / 2 + p of its slot's accumulator in LDS, which it
//                 alone owns.  Inactive slots and lanes r >= n add nothing, by a branch.  The slots are summed in order at the
//                 end.  Every LDS exchange is wave-private (wave_sync_lds); the one block barrier stands before the slot sum.
// Both: transposed partials [column][block], launch_ltm_final with scale 1, no atomics; the launch geometry is a function of
// the problem's sizes alone, so two calls return the same bits.  No register array is indexed at run time.
#include <algorithm>
#include <cstring>
#include <vector>

#include "ltm_eig_device.h"

namespace abz {

namespace {

struct LtmDensArgs {
    PlaneView H;  // H planes of the grid (full or Hermitian-compact); not read for one band
    PlaneView W;  // the resident weights: nE n planes per tile
    int64_t nlines;
    int n, npt;
    int e0;           // first energy of this launch (lane kernels; the row kernels take blockIdx.y)
    int ncol;         // columns per energy
    double* partial;  // [nE ncol][nrows]
    int64_t nrows;
};

template <int N, int NE>
__global__ __launch_bounds__(256) void ltm_dens_lane_kernel(LtmDensArgs a) {
    constexpr int NC = N * N;
    __shared__ double red[4][NE * NC];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = a.W.row;
    const int64_t total = a.nlines * row;
    double acc[NE][NC];
#pragma unroll
    for (int e = 0; e < NE; ++e) {
#pragma unroll
        for (int c = 0; c < NC; ++c) acc[e][c] = 0.0;
    }
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t line = t <= 0xffffffffll ? (int64_t)((uint32_t)t / (uint32_t)row) : t / row;
        const int i = (int)(t - line * row);
        if (i >= a.npt) continue;
        double ur[N][N], ui[N][N];  // [band][orbital]
        if constexpr (N == 1) {
            ur[0][0] = 1.0;
            ui[0][0] = 0.0;
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
        const double* __restrict__ const wp = a.W.base + line * a.W.tile + (int64_t)a.e0 * N * a.W.pitch + i;
#pragma unroll
        for (int e = 0; e < NE; ++e) {
#pragma unroll
            for (int b = 0; b < N; ++b) {
                const double w = wp[(int64_t)(e * N + b) * a.W.pitch];
#pragma unroll
                for (int p = 0; p < N; ++p) acc[e][p] += w * proj_diag(ur[b][p], ui[b][p]);
                int c = N;
#pragma unroll
                for (int p = 0; p < N; ++p) {
#pragma unroll
                    for (int q = p + 1; q < N; ++q) {
                        acc[e][c] += w * proj_re(ur[b][p], ui[b][p], ur[b][q], ui[b][q]);
                        acc[e][c + 1] += w * proj_im(ur[b][p], ui[b][p], ur[b][q], ui[b][q]);
                        c += 2;
                    }
                }
            }
        }
    }
    // every lane ends with the same bits: a + b == b + a at every level of the butterfly
#pragma unroll
    for (int e = 0; e < NE; ++e) {
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            double v = acc[e][c];
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
            if (lane == 0) red[wave][e * NC + c] = v;
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < NE * NC) {
        const int c = (int)threadIdx.x;
        a.partial[((int64_t)a.e0 * NC + c) * a.nrows + blockIdx.x] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

template <int NP>
__global__ __launch_bounds__(256, NP <= 16 ? 2 : 1) void ltm_dens_rows_kernel(LtmDensArgs a) {
    extern __shared__ double2 lds_dens[];
    constexpr int SLOTS = 256 / NP;
    constexpr int HALF = NP / 2;
    constexpr int RS = NP + 1;  // row stride of the transposed half of U
    static_assert(HALF * RS <= PARK_STRIDE<NP>, "half of U fits the reflector room");
    const int slot = threadIdx.x / NP, r0 = threadIdx.x % NP;
    double2* const acc = lds_dens + (size_t)(SLOTS + slot) * PARK_STRIDE<NP>;   // this slot's upper triangle, entry q (q + 1) / 2 + p
    double* const wts = reinterpret_cast<double*>(lds_dens + (size_t)2 * SLOTS * PARK_STRIDE<NP>) + slot * NP;  // w_b of this node
    const int npt = a.npt;
    const int iE = (int)blockIdx.y;
    // lane q owns the entries (p, q), p <= q, of its slot
    for (int p = 0; p <= r0; ++p) acc[r0 * (r0 + 1) / 2 + p] = make_double2(0.0, 0.0);
    for (int64_t item = blockIdx.x; item < a.nlines * rows_passes_per_line<NP>(npt); item += gridDim.x) {
        const RowsPass<NP> ps = rows_pass<NP>(lds_dens, item, npt, a.n);
        const int n = ps.n, r = ps.r;
        double2* const park = ps.park;  // this node's reflectors, then half of U
        if (!ps.wave_on) continue;      // a wave without a node has nothing to add
        double hr[NP], hi[NP];
        // herm_row_load written out (see there: behind the call this kernel's results move in the last bit at NP = 16)
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
        rows_eigh_columns<NP>(n, r, ps.lane, park, hr, hi, myeig, ur, ui);
        const bool mine = ps.act && r < n;  // this lane holds column r of a node of the grid
        wave_sync_lds();  // the back-transformation has read the reflectors: the room is free
        wts[r] = mine ? a.W.base[ps.line * a.W.tile + (int64_t)(iE * n + r) * a.W.pitch + ps.i1] : 0.0;
        // U through the room in two halves of the orbital index, the upper one first: the lanes of the half take their own row,
        // scaled by the weights of its bands, into registers, and every lane q forms (p, q) for the p <= q of the half
        double vr[NP], vi[NP];
#pragma unroll
        for (int h = 1; h >= 0; --h) {
#pragma unroll
            for (int pp = 0; pp < HALF; ++pp) park[pp * RS + r] = mine ? make_double2(ur[h * HALF + pp], ui[h * HALF + pp]) : make_double2(0.0, 0.0);
            wave_sync_lds();
            if (r / HALF == h) {
#pragma unroll
                for (int b = 0; b < NP; ++b) {
                    const double2 x = park[(r - h * HALF) * RS + b];
                    const double w = wts[b];
                    vr[b] = w * x.x;
                    vi[b] = w * x.y;
                }
            }
            if (mine) {
#pragma unroll 1
                for (int pp = 0; pp < HALF; ++pp) {
                    const int p = h * HALF + pp;
                    if (p > r) break;
                    const double2* __restrict__ const xp = park + pp * RS;
                    double sr = 0.0, si = 0.0;
#pragma unroll
                    for (int b = 0; b < NP; ++b) {
                        if (b < n) {  // uniform
                            const double2 x = xp[b];
                            sr += proj_re(x.x, x.y, vr[b], vi[b]);
                            si += proj_im(x.x, x.y, vr[b], vi[b]);
                        }
                    }
                    double2 s = acc[r * (r + 1) / 2 + p];
                    s.x += sr;
                    s.y += p == r ? 0.0 : si;
                    acc[r * (r + 1) / 2 + p] = s;
                }
            }
            wave_sync_lds();  // the half was read: the room and the weights are free
        }
    }
    __syncthreads();
    // the slots in order
    const int npair = a.n * (a.n + 1) / 2;
    const double2* const acc0 = lds_dens + (size_t)SLOTS * PARK_STRIDE<NP>;
    for (int idx = threadIdx.x; idx < npair; idx += 256) {
        double sr = 0.0, si = 0.0;
        for (int s = 0; s < SLOTS; ++s) {
            const double2 x = acc0[(size_t)s * PARK_STRIDE<NP> + idx];
            sr += x.x;
            si += x.y;
        }
        double* __restrict__ const out = a.partial + ((int64_t)iE * a.ncol + 2 * idx) * a.nrows + blockIdx.x;
        out[0] = sr;
        out[a.nrows] = si;
    }
}

}  // namespace

// out_host [nE][n][n][2] = rho(E_i) per unit cell from the weights W (nE energies) and the H planes; the lower triangle is the exact
// conjugate of the upper one.  One synchronisation.
int launch_ltm_density_matrix(abz_ctx* ctx, int n, int npt, int64_t nlines, PlaneView H, PlaneView W, int nE, double* out_host) {
    const bool lanes = n <= 4;
    const int ncol = lanes ? n * n : n * (n + 1);  // lanes: diagonal, then (Re, Im) of p < q; rows: (Re, Im) of entry q (q + 1) / 2 + p
    const int ntot = nE * ncol;
    int64_t nblocks;
    int np = 0;
    if (lanes) {
        nblocks = std::max<int64_t>(1, std::min<int64_t>((nlines * W.row + 255) / 256, 2048));
    } else {
        np = rows_np(n);
        nblocks = std::max<int64_t>(1, rows_blocks(np, npt, nlines, std::max(128, 1024 / nE)));
    }
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nblocks * (size_t)ntot);
    if (rc) return rc;
    // the columns travel as pairs of doubles: the mailbox and its fallback speak double2
    const int64_t npair = (ntot + 1) / 2;
    std::vector<double> cols(2 * (size_t)npair);
    const SumOut so = sum_out_mailbox(ctx, cols.data(), (size_t)npair);
    double2* where = nullptr;
    if ((rc = sum_target(ctx, so, 0, npair, &where))) return rc;
    LtmDensArgs a;
    a.H = H;
    a.W = W;
    a.nlines = nlines;
    a.n = n;
    a.npt = npt;
    a.e0 = 0;
    a.ncol = ncol;
    a.partial = ctx->scratch[1].as<double>();
    a.nrows = nblocks;
    {
        ProfScope ps(ctx, ABZ_K_EIG);
        if (lanes) {
            // groups of 4 energies, then single ones: the solve of a node serves the group
            for (int i0 = 0; i0 < nE;) {
                const int ne = nE - i0 >= 4 ? 4 : 1;
                a.e0 = i0;
                const dim3 grid((unsigned)nblocks);
                lanes_dispatch(n, [&](auto N) {
                    launch(ctx, ne == 1 ? ltm_dens_lane_kernel<decltype(N)::value, 1> : ltm_dens_lane_kernel<decltype(N)::value, 4>, grid, dim3(256), 0, a);
                    return ABZ_OK;
                });
                i0 += ne;
            }
        } else {
            // its own grid: blockIdx.y = energy.  Behind the rooms: as much again for the slots' accumulators, and 256 weights
            const size_t lds = rows_lds_bytes(np, rows_room_bytes(np) + sizeof(double) * 256);
            const dim3 grid((unsigned)nblocks, (unsigned)nE);
            if ((rc = rows_dispatch(np, [&](auto NP) { return launch_rows(ctx, ltm_dens_rows_kernel<decltype(NP)::value>, grid, lds, a); }))) return rc;
        }
        ABZ_HIP(hipGetLastError());
    }
    {
        ProfScope ps(ctx, ABZ_K_LTM);
        // column by column as they are (scale 1: x to the bit)
        if ((rc = launch_ltm_final(ctx, a.partial, nblocks, 1.0, ntot, ntot, 0, reinterpret_cast<double*>(where)))) return rc;
    }
    if ((rc = sum_deliver(ctx, so, where, 0, npair))) return rc;
    for (int i = 0; i < nE; ++i) {
        const double* c = cols.data() + (size_t)i * ncol;
        double* o = out_host + (size_t)i * n * n * 2;
        int k = n;
        for (int p = 0; p < n; ++p) {
            for (int q = p; q < n; ++q) {
                double re, im;
                if (lanes) {
                    re = p == q ? c[p] : c[k];
                    im = p == q ? 0.0 : c[k + 1];
                    if (p != q) k += 2;
                } else {
                    const int idx = q * (q + 1) / 2 + p;
                    re = c[2 * idx];
                    im = p == q ? 0.0 : c[2 * idx + 1];
                }
                o[2 * (p * n + q)] = re;
                o[2 * (p * n + q) + 1] = im;
                o[2 * (q * n + p)] = re;
                o[2 * (q * n + p) + 1] = p == q ? 0.0 : -im;
            }
        }
    }
    return ABZ_OK;
}

}  // namespace abz
