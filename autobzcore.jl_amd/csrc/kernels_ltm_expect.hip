// Band expectation values of operator series as matrix elements of the tetrahedron method (abz_rule_ltm_expectation):
//   q_i(b, k) = Re u_b(k)^H Hermitian(O_i(k)) u_b(k),   component c = q_i (single) or q_i q_j (product),
// the H planes of a whole periodic grid and the planes of up to ABZ_LTM_EXPECT_MAX_OPS operator rules of the same grid in,
// the element block of abz_rule_ltm_elements out (plane c n + b of a grid line's tile, padded rows, the padding columns
// written as zeros).  Loads, pass head, write-out and launch are the frame of ltm_eig_device.h.  Neither U nor O u reaches HBM,
// no atomics, no dependence on the launch geometry: two calls write the same bits.
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
#include "ltm_eig_device.h"

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
            CMat<N> h;
            herm_lane_load<N>(a.H, line, i, h);
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
                    const int64_t pl = herm_plane(O, N, p, s);
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
    double* const tile = reinterpret_cast<double*>(lds_xp + SLOTS * PARK_STRIDE<NP>);  // [component][NP bands][TS]
    const int npt = a.npt, nplanes = a.ncomp * a.n;
    for (int64_t item = blockIdx.x; item < a.nlines * rows_passes_per_line<NP>(npt); item += gridDim.x) {
        const RowsPass<NP> ps = rows_pass<NP>(lds_xp, item, npt, a.n);  // ps.park: the node's reflectors, then its operator
        const int n = ps.n, r = ps.r;
        if (ps.wave_on) {
            const int column = ps.act ? ps.i1 : 0;
            double hr[NP], hi[NP];
            // (a local closure over the shared load, as in kernels_ltm_pairs.hip: the register counts are the ones these
            // kernels had with their own closures)
            auto load_row = [&](const PlaneView& X) { herm_row_load<NP>(X, n, r, ps.line, column, hr, hi); };
            load_row(a.H);
            double myeig, ur[NP], ui[NP];
            rows_eigh_columns<NP>(n, r, ps.lane, ps.park, hr, hi, myeig, ur, ui);
            double q[XOPS];
#pragma unroll
            for (int m = 0; m < XOPS; ++m) q[m] = 0.0;
            for (int k = 0; k < a.nops; ++k) {  // (uniform)
                load_row(a.O[k]);
                wave_sync_lds();  // every lane of the node is done reading the room (reflectors, the operator before)
                park_upper<NP>(n, r, ps.park, hr, hi);
                wave_sync_lds();
                const double v = quad_form<NP>(n, ps.park, ur, ui, std::make_integer_sequence<int, NP>());
                xp_put(q, k, v);
            }
            if (ps.act && r < n) {
                for (int c = 0; c < a.ncomp; ++c) {
                    const int ki = a.ci[c], kj = a.cj[c];  // (uniform)
                    const double x = xp_pick(q, ki);
                    tile[(c * NP + r) * TS + ps.slot] = kj < 0 ? x : x * xp_pick(q, kj);
                }
            }
        }
        __syncthreads();
        rows_tile_write<NP>(a.A, ps.line, ps.i0, npt, a.n, nplanes, tile, [](int c, int b) { return c * NP + b; });
        __syncthreads();  // the tile is free for the next pass
    }
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
    int rc;
    if (n <= 4) {
        rc = lanes_dispatch(n, [&](auto N) { return launch_lanes(ctx, ltm_expect_lane_kernel<decltype(N)::value>, nlines, A.row, a); });
    } else {
        const int np = rows_np(n);
        const size_t lds = rows_lds_bytes(np, rows_tile_bytes(np, ncomp));
        const dim3 grid((unsigned)rows_blocks(np, npt, nlines, 256 * 64));
        rc = rows_dispatch(np, [&](auto NP) { return launch_rows(ctx, ltm_expect_rows_kernel<decltype(NP)::value>, grid, lds, a); });
    }
    if (rc) return rc;
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
