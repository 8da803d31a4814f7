// Optimized tetrahedron method (gfx950 only): g(E), N(E), g_A(E), N_A(E) from the cached eigenvalues of a full 3-d grid with the
// leading O(1/npt^2) interpolation error of the linear method removed.
//
// Kawamura, Gohda, Tsuneyuki, PRB 89, 094515 (2014).  The reference has no counterpart (src/dos_algorithms.jl:1-7 plans "LTM").
//
//  * Definition (d = 3).  A Kuhn simplex of cell i is the path v1 = i (corner 0), v2 = v1 + e_a, v3 = v2 + e_b, v4 = v3 + e_c (corner 7)
//    over a permutation (a, b, c) of the axes: the six (0, a, b, 7) of kernels_ltm.hip.  The band is taken at 20 grid points,
//      p1..p4   = v1..v4
//      p5..p16  = 2 v_i - v_j,  (i, j) = (1,2) (2,3) (3,4) (4,1) (1,3) (2,4) (3,1) (4,2) (1,4) (2,1) (3,2) (4,3)
//      p17..p20 = v4 - v1 + v2,  v1 - v2 + v3,  v2 - v3 + v4,  v3 - v4 + v1,
//    all inside i + [-1, 2]^3, every index wrapped mod npt (any npt >= 1; below 4 the stencil wraps onto itself).  The cubic through
//    the 20 values is fitted, and the 4 corner values are replaced by those of the linear function closest to it in the
//    least-squares sense over the simplex: x'_m = sum_j P[m][j] x(p_j), OPT_K = 1260 P in ltm_opt_device.h (rows sum to 1260; derived in exact
//    rationals by tests/optltm_numpy.py, which does not read this table).  For band b, x is the b-th ascending eigenvalue at each
//    point (no band unfolding); elements A_b take the same P at the same points.  Every closed form of the linear method
//    (ltm_simplex_device.h) then applies unchanged to (e'_1..e'_4; A'_1..A'_4), with the weight 1 / (6 npt^3) per simplex; a simplex
//    wholly below E adds the mean of its A' to the step histogram at the first energy >= max e'.
//  * Rows sum to one, so x'_m = x_m + sum_{j != m} P[m][j] (x_j - x_m): this is the form evaluated.  A flat band keeps its value
//    to the bit (g = 0, a unit step), A = 1 gives A' = 1 exactly, and the rounding error scales with the variation of the band
//    over the stencil instead of its absolute value.
//  * Shape (ltm_opt_kernel<STATES, SRC, NC>).  Energies ascending in LDS, blockIdx.y the band, one histogram per wave and kind,
//    fixed-order reduction into transposed partials, then ltm_final_kernel / ltm_prefix_kernel of kernels_ltm.hip as they are:
//    two calls return the same bits.  A block walks 256 cells at a time, one cell per thread, and every thread takes the six
//    simplices of its cell one after the other: the permutation is uniform over the wave, so the 20 loads of a simplex are 20
//    shifted copies of the same run of a grid line (consecutive lanes, consecutive i_1), and the 4^3 neighbourhood that the six
//    simplices and the neighbouring cells share is served by the caches.  Per axis the thread keeps the 4 wrapped indices
//    i - 1 .. i + 2 as (column, line) contributions; a simplex picks its three tables by compares on the permutation and every
//    point is three constant-index entries of them: nothing is indexed by a run-time value, nothing goes to scratch.  This
//    addressing is OptPath of ltm_opt_device.h, which every kernel of the optimized rule uses; the header also has what this
//    scan shares with ltm_green_opt_kernel: the sources, the shared arguments, the band's planes (OptBand), the effective
//    elements of a simplex (opt_elements) and the opening of the launcher (opt_scan_open).
//  * Window.  e' can leave the range of the cell's 8 corners (sum_j |P[m][j]| = 1836 / 1260), so the window [min e', max e') is
//    that of the effective energies of each simplex, taken after the product.  A simplex with no energy at or above min e' is
//    done; without STATES one with no energy below max e' too, before its elements are loaded.  Everything else goes to
//    ltm_simplex3 of the element payload, which walks the energies of the window and places the step.  There is no queue: the
//    20 loads and the 4 x 17 product of every simplex come before the window is known, and they, not the walk, set the time
//    (DESIGN section 4e).
//  * Sources.  OPT_ONE: A' = 1, nothing loaded.  OPT_ENERGY: A' = e', nothing loaded.  OPT_ELEMS: NC = 1, 2 or 4 components per
//    launch, 20 loads and one product per component, after the window test.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_opt_device.h"
#include "ltm_simplex_device.h"

namespace abz {

namespace {

struct OptArgs : OptScanArgs {
    const double* Es;  // device, ascending
    int nE;
    double inv_step = 0.0;
};

// what ltm_simplex3 asks of its payload
template <int NC_>
struct OptPayload {
    static constexpr int NC = NC_;
    static constexpr bool CORR = false;
};

// partial [(STATES ? 2 : 1) NC nE][nrows]: columns c nE + i the formula sums of component c, NC nE + c nE + i its steps
template <bool STATES, int SRC, int NC>
__global__ __launch_bounds__(256) void ltm_opt_kernel(OptArgs a, double* __restrict__ partial, int64_t nrows) {
    static_assert(SRC == OPT_ELEMS || NC == 1, "one component without attached elements");
    // [nE] energies | [4 waves][NC][nE] sums | STATES: [4 waves][NC][nE] steps
    extern __shared__ __attribute__((aligned(16))) double ldsl[];
    using Pay = OptPayload<NC>;
    using Vec = LtmVec<NC>;
    const int wave = threadIdx.x >> 6;
    const int nE = a.nE;
    constexpr int NH = (STATES ? 8 : 4) * NC;
    const double* const Esl = ldsl;
    double* const hist = ldsl + (size_t)(1 + wave * NC) * nE;
    double* const step = ldsl + (size_t)(1 + (4 + wave) * NC) * nE;  // STATES only
    for (int i = threadIdx.x; i < nE; i += 256) ldsl[i] = a.Es[i];
    for (int i = threadIdx.x; i < NH * nE; i += 256) ldsl[nE + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const OptBand<SRC> band(a);
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        if (k >= a.ncell) continue;  // (no barrier inside the walk)
        const LtmCell cell = ltm_cell<3>(k, npt);
        int j1[4], j2[4], j3[4];
        opt_tables(cell.i1, cell.i2, cell.i3, npt, j1, j2, j3);
#pragma unroll 1
        for (int t = 0; t < 6; ++t) {
            const OptPath path(t, j1, j2, j3);
            double x[OPT_NPT], e[4];
            path.load(band.Eb, band.tileE, x);
            opt_project(x, e);
            const double emin = fmin(fmin(e[0], e[1]), fmin(e[2], e[3])), emax = fmax(fmax(e[0], e[1]), fmax(e[2], e[3]));
            const int i0 = ltm_first(Esl, nE, a.inv_step, emin);
            if (i0 >= nE) continue;                       // every energy lies below the simplex
            if (!STATES && !(Esl[i0] < emax)) continue;   // no energy inside the window: nothing for g
            Vec A[4];
            opt_elements<SRC, NC>(path, band, e, A);
            ltm_simplex3<STATES, Pay>(e[0], e[1], e[2], e[3], A[0], A[1], A[2], A[3], Esl, nE, i0, hist, step);
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = ldsl + nE;
    // transposed partials [column][row], as ltm_window_kernel writes them
    for (int t = threadIdx.x; t < NC * nE; t += 256) {
        const size_t w = (size_t)NC * nE;  // from one wave's histograms to the next
        partial[(int64_t)t * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
        if (STATES) partial[((int64_t)NC * nE + t) * nrows + prow] = (h[4 * w + t] + h[5 * w + t]) + (h[6 * w + t] + h[7 * w + t]);
    }
}

using OptFn = void (*)(abz_ctx*, dim3, size_t, const OptArgs&, double*, int64_t);
template <bool STATES, int SRC, int NC>
void opt_launch(abz_ctx* ctx, dim3 grid, size_t lds, const OptArgs& a, double* partial, int64_t nrows) {
    launch(ctx, (ltm_opt_kernel<STATES, SRC, NC>), grid, dim3(256), (unsigned)lds, a, partial, nrows);
}

// the compiled kernels: [states][source][NC]
OptFn opt_fn(bool states, int src, int nc) {
    if (src == OPT_ONE) return states ? opt_launch<true, OPT_ONE, 1> : opt_launch<false, OPT_ONE, 1>;
    if (src == OPT_ENERGY) return states ? opt_launch<true, OPT_ENERGY, 1> : opt_launch<false, OPT_ENERGY, 1>;
    switch (nc) {
        case 1: return states ? opt_launch<true, OPT_ELEMS, 1> : opt_launch<false, OPT_ELEMS, 1>;
        case 2: return states ? opt_launch<true, OPT_ELEMS, 2> : opt_launch<false, OPT_ELEMS, 2>;
        case 4: return states ? opt_launch<true, OPT_ELEMS, 4> : opt_launch<false, OPT_ELEMS, 4>;
    }
    return nullptr;
}

}  // namespace

// The host side of ltm_scan (kernels_ltm.hip) for the optimized kernel: chunks of energies, groups of 4, 2, 1 components, the same
// final and prefix kernels.  A == nullptr: one component, A = 1 (`energy` false) or A = e (`energy` true).
int launch_ltm_optimized(abz_ctx* ctx, int n, int npt, PlaneView E, const PlaneView* A, bool energy, int ncomp, const double* Es_host, int nE,
                         bool states, double* out_host) {
    OptArgs a;
    int src;
    int64_t nblocks, nrows;
    int rc = opt_scan_open("abz_rule_ltm_optimized", n, npt, E, A, energy, ncomp, a, src, nblocks, nrows);
    if (rc) return rc;
    const double weight = 1.0 / (6.0 * (double)a.ncell);
    const int ncol = states ? 2 : 1;
    // energies per launch of NC components, as in ltm_scan: 8 (1 + 4 NC ncol) B of LDS each within LTM_LDS_MAX, at most 512 where
    // the prefix kernel holds a chunk's steps
    auto chunk = [&](int nc) {
        const size_t fit = LTM_LDS_MAX / (sizeof(double) * (size_t)(1 + 4 * nc * ncol));
        return (int)std::min<size_t>(fit, states ? 512 : 1024);
    };
    size_t pmax = 0;
    for (int nc : {1, 2, 4})
        if (nc <= ncomp) pmax = std::max(pmax, (size_t)std::min(nE, chunk(nc)) * (size_t)(nc * ncol));
    if ((rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nrows * pmax))) return rc;
    double* partial = ctx->scratch[1].as<double>();
    EnergyList el;
    // behind the energies: the column sums of a launch, [nc][cnt] sums | [nc][cnt] steps (states)
    if ((rc = energies_to_device(ctx, Es_host, nE, true, 2 * 4 * (size_t)512, el, ncomp))) return rc;
    double* col = el.extra;
    a.inv_step = el.inv_step;
    const dim3 grid((unsigned)nblocks, (unsigned)n);
    for (int c0 = 0; c0 < ncomp;) {
        const int nc = ncomp - c0 >= 4 ? 4 : (ncomp - c0 >= 2 ? 2 : 1);
        const int CH = chunk(nc);
        const OptFn fn = opt_fn(states, src, nc);
        a.aplane0 = c0 * n;
        for (int s0 = 0; s0 < nE; s0 += CH) {
            const int cnt = std::min(CH, nE - s0);
            a.Es = el.dev + s0;
            a.nE = cnt;
            ProfScope ps(ctx, ABZ_K_LTM);
            const size_t lds = sizeof(double) * (size_t)(1 + 4 * nc * ncol) * (size_t)cnt;
            double* const o = el.out + (size_t)c0 * nE + s0;  // results [ncomp][nE] in sorted order
            fn(ctx, grid, lds, a, partial, nrows);
            ABZ_HIP(hipGetLastError());
            if (states) {
                if ((rc = launch_ltm_final(ctx, partial, nrows, 1.0, 2 * nc * cnt, 2 * nc * cnt, 0, col))) return rc;
                if ((rc = launch_ltm_prefix(ctx, col, cnt, nc, weight, (int64_t)nE, o))) return rc;
            } else if ((rc = launch_ltm_final(ctx, partial, nrows, weight, nc * cnt, cnt, nE, o))) {
                return rc;
            }
        }
        c0 += nc;
    }
    return energies_deliver(ctx, el, out_host);
}

}  // namespace abz
