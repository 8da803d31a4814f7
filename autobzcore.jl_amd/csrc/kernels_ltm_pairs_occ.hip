// Interband spectra of a metal (abz_rule_ltm_pairs_occupied, gfx950 only): the scans of a pair rule with the T = 0 occupation
// factor theta(E_F - e_v) theta(e_c - E_F) inside every simplex,
//   J^occ(w)    = w_s sum_vc sum_simplices int theta(E_F - e_v) theta(e_c - E_F) delta(w - Delta_vc) dk
//   S^occ_ij(w) = the same with the attached interband products A^{ij}_vc(k) under the integral,
// and their cumulative forms (theta(w - Delta) for delta), w_s = 1 / (d! npt^d).  Inside a simplex e_v, e_c and Delta = e_c - e_v are
// all linear, so the region {e_v <= E_F} and {e_c > E_F} is the simplex cut by two planes, a union of sub-simplices on which
// the closed forms of the plain scans apply (ltm_simplex1/2/3 of ltm_simplex_device.h, unchanged): a sub-simplex with
// barycentric corner matrix B is passed with the corner energies B Delta and the corner elements |det B| (B A) -- the sums are linear
// in A, so the volume fraction rides in the elements.  A = 1 (ABZ_LTM_A_ONE) is one component of ones.
//  * Shape: that of ltm_window_kernel (kernels_ltm.hip) without its queue.  The energies are ascending and live in LDS; blockIdx.y
//    is the pseudo-band p of the pair rule, v = v0 + p / nc, c = c0 + p % nc; a thread takes one cell at a time.  The corner
//    energies e_v, e_c come from the SOURCE's planes (the pair rule's Delta planes are never read: Delta is formed here by the same one
//    subtraction), the corner elements from plane aplane0 + p of the pair rule's element block.  Per-wave histograms, transposed
//    partials, ltm_final_kernel / ltm_prefix_kernel, component groups of 4, 2, 1 and the energy chunks are those of ltm_scan.
//  * Per cell: no corner with e_v <= E_F, or none with e_c > E_F: nothing.  Every energy below the cell's Delta range: nothing.
//    All corners occupied in v and empty in c (an uncut cell) and no energy inside the range: one add of the corner means to
//    the step histogram, as in the plain scan.  That shortcut holds for an uncut cell only: a cut cell below w steps by the
//    integral of A over its occupied part, so it walks its simplices.
//  * Per simplex (a run-time loop over the d! Kuhn simplices; the corners are read again per simplex, from L1/L2, so that no
//    register array is indexed at run time): sort the corners by e_v, m = corners with e_v <= E_F.
//        d = 3   m = 1  the tip        (0, P01, P02, P03)                                              volume t01 t02 t03
//                m = 2  the prism      (0, P02, P03, 1) (P02, P03, 1, P12) (P03, 1, P12, P13)          t02 t03 | (1-t02) t03 t12 | (1-t03) t12 t13
//                m = 3  the frustum    (0, 1, 2, P03) (1, 2, P03, P13) (2, P03, P13, P23)              t03 | (1-t03) t13 | (1-t03)(1-t13) t23
//                m = 4  the simplex itself
//        d = 2   m = 1  (0, P01, P02)  t01 t02;     m = 2  (1, 0, P12) (0, P12, P02)  t12 | (1-t12) t02;     m = 3 itself
//        d = 1   m = 1  (0, P01)  t01;     m = 2 itself
//    P_ij the point of edge i-j on the plane, t_ij = (E_F - k_i) / (k_j - k_i) in [0, 1] with k_i <= E_F < k_j: no division by
//    zero.  Every piece is then sorted by -e_c and cut the same way by -e_c < -E_F.  All volumes are products of numbers in
//    [0, 1]: a POSITIVE decomposition, nothing cancels when two corner energies nearly coincide.  The pieces of a cut are
//    consecutive windows of d + 1 points of one list of at most 2 d, so one run-time loop slides a window over it and the
//    closed form has ONE call site per kernel.
//  * Ties follow the scans' half-open rule (N(E) counts e <= E): a corner is occupied iff e_v <= E_F, empty iff e_c > E_F.
//  * i0 and the activity test use the cell's Delta range; a sub-simplex's range lies inside it and the closed forms walk from i0.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_simplex_device.h"

namespace abz {

namespace {

struct LtmOccArgs {
    PlaneView E;       // the eigenvalue planes of the SOURCE rule
    PlaneView A;       // the element block of the pair rule; base == nullptr: A = 1
    const double* Es;  // device, ascending
    int64_t ncell;     // npt^d
    int64_t acomp;     // doubles from a pseudo-band's plane of one component to its plane of the next: nb * A.pitch
    int npt, nE;
    int aplane0;       // first element plane of this launch: (its first component) * nb
    int v0, c0, pnc;   // pseudo-band p: v = v0 + p / pnc, c = c0 + p % pnc
    double EF;
    double inv_step = 0.0;
};

// what ltm_simplex1/2/3 ask of a payload
template <int NC_>
struct OccElems {
    static constexpr int NC = NC_;
    static constexpr bool CORR = false;
};

// A vertex of a (sub-)simplex: the key of the cut at hand (e_v, then -e_c), e_c carried through the first cut, Delta, the elements.
template <int NC>
struct OccVert {
    double k, ec, dl;
    LtmVec<NC> A;
};

template <int NC>
__device__ __forceinline__ OccVert<NC> occ_lerp(const OccVert<NC>& a, const OccVert<NC>& b, double t) {
    OccVert<NC> r;
    r.k = fma(t, b.k - a.k, a.k);
    r.ec = fma(t, b.ec - a.ec, a.ec);
    r.dl = fma(t, b.dl - a.dl, a.dl);
#pragma unroll
    for (int c = 0; c < NC; ++c) r.A.v[c] = fma(t, b.A.v[c] - a.A.v[c], a.A.v[c]);
    return r;
}

template <int NC>
__device__ __forceinline__ OccVert<NC> occ_pick(bool second, const OccVert<NC>& a, const OccVert<NC>& b) {
    OccVert<NC> r;
    r.k = second ? b.k : a.k;
    r.ec = second ? b.ec : a.ec;
    r.dl = second ? b.dl : a.dl;
#pragma unroll
    for (int c = 0; c < NC; ++c) r.A.v[c] = second ? b.A.v[c] : a.A.v[c];
    return r;
}

// compare-exchange by the key
template <int NC>
__device__ __forceinline__ void occ_cx(OccVert<NC>& a, OccVert<NC>& b) {
    const bool sw = b.k < a.k;
    const OccVert<NC> lo = occ_pick(sw, a, b), hi = occ_pick(sw, b, a);
    a = lo;
    b = hi;
}

template <int D, int NC>
__device__ __forceinline__ void occ_sort(OccVert<NC> (&v)[D + 1]) {
    if constexpr (D == 3) {
        occ_cx(v[0], v[1]);
        occ_cx(v[2], v[3]);
        occ_cx(v[0], v[2]);
        occ_cx(v[1], v[3]);
        occ_cx(v[1], v[2]);
    } else if constexpr (D == 2) {
        occ_cx(v[0], v[1]);
        occ_cx(v[1], v[2]);
        occ_cx(v[0], v[1]);
    } else {
        occ_cx(v[0], v[1]);
    }
}

// The part of a simplex on the inner side of a plane.  v: the corners in ascending order of the key, the first m of them inside
// (k_i <= F or k_i < F, the caller's rule; every other corner has k_j >= F resp. > F, so k_j - k_i > 0 wherever it is divided by).
// -> the number of pieces; piece p has the vertices s[p .. p + D] and the volume fraction vol[p].
template <int D, int NC>
__device__ __forceinline__ int occ_clip(const OccVert<NC> (&v)[D + 1], int m, double F, OccVert<NC> (&s)[2 * D], double (&vol)[D]) {
#pragma unroll
    for (int j = 0; j < 2 * D; ++j) s[j] = v[j <= D ? j : D];
    vol[0] = 1.0;
#pragma unroll
    for (int j = 1; j < D; ++j) vol[j] = 0.0;
    if (m <= 0) return 0;
    if (m > D) return 1;
    auto t = [&](int i, int j) { return (F - v[i].k) / (v[j].k - v[i].k); };
    if constexpr (D == 1) {
        const double t01 = t(0, 1);
        s[1] = occ_lerp(v[0], v[1], t01);
        vol[0] = t01;
        return 1;
    } else if constexpr (D == 2) {
        if (m == 1) {
            const double t01 = t(0, 1), t02 = t(0, 2);
            s[1] = occ_lerp(v[0], v[1], t01);
            s[2] = occ_lerp(v[0], v[2], t02);
            vol[0] = t01 * t02;
            return 1;
        }
        const double t02 = t(0, 2), t12 = t(1, 2);
        s[0] = v[1];
        s[1] = v[0];
        s[2] = occ_lerp(v[1], v[2], t12);
        s[3] = occ_lerp(v[0], v[2], t02);
        vol[0] = t12;
        vol[1] = (1.0 - t12) * t02;
        return 2;
    } else {
        if (m == 1) {
            const double t01 = t(0, 1), t02 = t(0, 2), t03 = t(0, 3);
            s[1] = occ_lerp(v[0], v[1], t01);
            s[2] = occ_lerp(v[0], v[2], t02);
            s[3] = occ_lerp(v[0], v[3], t03);
            vol[0] = t01 * t02 * t03;
            return 1;
        }
        if (m == 2) {
            const double t02 = t(0, 2), t03 = t(0, 3), t12 = t(1, 2), t13 = t(1, 3);
            s[1] = occ_lerp(v[0], v[2], t02);
            s[2] = occ_lerp(v[0], v[3], t03);
            s[3] = v[1];
            s[4] = occ_lerp(v[1], v[2], t12);
            s[5] = occ_lerp(v[1], v[3], t13);
            vol[0] = t02 * t03;
            vol[1] = (1.0 - t02) * t03 * t12;
            vol[2] = (1.0 - t03) * t12 * t13;
            return 3;
        }
        const double t03 = t(0, 3), t13 = t(1, 3), t23 = t(2, 3);
        s[3] = occ_lerp(v[0], v[3], t03);
        s[4] = occ_lerp(v[1], v[3], t13);
        s[5] = occ_lerp(v[2], v[3], t23);
        vol[0] = t03;
        vol[1] = (1.0 - t03) * t13;
        vol[2] = (1.0 - t03) * (1.0 - t13) * t23;
        return 3;
    }
}

// the window of piece p >= 1 from the window of piece p - 1: drop the first vertex, take s[D + p] (selects, no run-time index)
template <int D, int NC>
__device__ __forceinline__ void occ_slide(OccVert<NC> (&w)[D + 1], const OccVert<NC> (&s)[2 * D], int p) {
#pragma unroll
    for (int j = 0; j < D; ++j) w[j] = w[j + 1];
    if constexpr (D == 3) w[D] = occ_pick(p == 1, s[5], s[4]);
    else w[D] = s[2 * D - 1];
}

// (written out per D: a loop over the pieces here is unrolled too late for the array to leave scratch)
template <int D>
__device__ __forceinline__ double occ_vol(const double (&vol)[D], int p) {
    if constexpr (D == 3) return p == 1 ? vol[1] : (p == 2 ? vol[2] : vol[0]);
    else if constexpr (D == 2) return p == 1 ? vol[1] : vol[0];
    else return vol[0];
}

// One Kuhn simplex: v[j].k = e_v, .ec = e_c, .dl = e_c - e_v, .A the elements of corner j, in any order.
template <int D, bool STATES, int NC>
__device__ __forceinline__ void occ_simplex(OccVert<NC> (&v)[D + 1], double EF, const double* Esl, int nE, int i0, double* hist, double* step) {
    occ_sort<D>(v);
    int m1 = 0;
#pragma unroll
    for (int j = 0; j <= D; ++j) m1 += v[j].k <= EF ? 1 : 0;
    OccVert<NC> s1[2 * D];
    double vol1[D];
    const int np1 = occ_clip<D>(v, m1, EF, s1, vol1);
    OccVert<NC> w[D + 1];
#pragma unroll
    for (int j = 0; j <= D; ++j) w[j] = s1[j];
#pragma unroll 1
    for (int p = 0; p < np1; ++p) {
        if (p > 0) occ_slide<D>(w, s1, p);
        const double f1 = occ_vol<D>(vol1, p);
        // the piece, keyed by -e_c; its volume fraction goes into the elements
        OccVert<NC> u[D + 1];
        int m2 = 0;
#pragma unroll
        for (int j = 0; j <= D; ++j) {
            u[j] = w[j];
            u[j].k = -w[j].ec;
            m2 += u[j].k < -EF ? 1 : 0;
#pragma unroll
            for (int c = 0; c < NC; ++c) u[j].A.v[c] = f1 * w[j].A.v[c];
        }
        if (m2 == 0) continue;
        occ_sort<D>(u);
        OccVert<NC> s2[2 * D];
        double vol2[D];
        const int np2 = occ_clip<D>(u, m2, -EF, s2, vol2);
        OccVert<NC> x[D + 1];
#pragma unroll
        for (int j = 0; j <= D; ++j) x[j] = s2[j];
#pragma unroll 1
        for (int q = 0; q < np2; ++q) {
            if (q > 0) occ_slide<D>(x, s2, q);
            const double f2 = occ_vol<D>(vol2, q);
            LtmVec<NC> B[D + 1];
#pragma unroll
            for (int j = 0; j <= D; ++j) {
#pragma unroll
                for (int c = 0; c < NC; ++c) B[j].v[c] = f2 * x[j].A.v[c];
            }
            if constexpr (D == 3)
                ltm_simplex3<STATES, OccElems<NC>>(x[0].dl, x[1].dl, x[2].dl, x[3].dl, B[0], B[1], B[2], B[3], Esl, nE, i0, hist, step);
            else if constexpr (D == 2)
                ltm_simplex2<STATES, OccElems<NC>>(x[0].dl, x[1].dl, x[2].dl, B[0], B[1], B[2], Esl, nE, i0, hist, step);
            else
                ltm_simplex1<STATES, OccElems<NC>>(x[0].dl, x[1].dl, B[0], B[1], Esl, nE, i0, hist, step);
        }
    }
}

// partial [(STATES ? 2 : 1) NC nE][nrows], as ltm_window_kernel leaves it
template <int D, bool STATES, int NC>
__global__ __launch_bounds__(256) void ltm_pairs_occ_kernel(LtmOccArgs a, double* __restrict__ partial, int64_t nrows) {
    // [nE] energies | [4 waves][NC][nE] sums | STATES: [4 waves][NC][nE] steps
    extern __shared__ __attribute__((aligned(16))) double lds_occ[];
    const int wave = threadIdx.x >> 6;
    const int nE = a.nE;
    constexpr int NH = (STATES ? 8 : 4) * NC;
    constexpr int NS = ltm_nsimplex(D);
    constexpr int NV = 1 << D;
    const double* const Esl = lds_occ;
    double* const hist = lds_occ + (size_t)(1 + wave * NC) * nE;
    double* const step = lds_occ + (size_t)(1 + (4 + wave) * NC) * nE;  // STATES only
    for (int i = threadIdx.x; i < nE; i += 256) lds_occ[i] = a.Es[i];
    for (int i = threadIdx.x; i < NH * nE; i += 256) lds_occ[nE + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const double EF = a.EF;
    const int p = (int)blockIdx.y;
    const double* __restrict__ const Evb = a.E.base + (int64_t)(a.v0 + p / a.pnc) * a.E.pitch;
    const double* __restrict__ const Ecb = a.E.base + (int64_t)(a.c0 + p % a.pnc) * a.E.pitch;
    const int64_t tileE = a.E.tile, tileA = a.A.tile, acomp = a.acomp;
    const bool ones = a.A.base == nullptr;  // (uniform)
    const double* __restrict__ const Ab = ones ? nullptr : a.A.base + (int64_t)(a.aplane0 + p) * a.A.pitch;
    // corner `bits` of cell (i1, i2, i3): e_v, e_c and the elements
    auto cornerV = [&](int i1, int i2, int i3, int bits) -> OccVert<NC> {
        ltm_wrap<D>(i1, i2, i3, bits, npt);
        const int64_t line = (int64_t)i3 * npt + i2;
        OccVert<NC> r;
        r.k = Evb[line * tileE + i1];
        r.ec = Ecb[line * tileE + i1];
        r.dl = r.ec - r.k;
        if (ones) {
#pragma unroll
            for (int c = 0; c < NC; ++c) r.A.v[c] = 1.0;
        } else {
            r.A = ltm_load<NC>(Ab + line * tileA + i1, acomp);
        }
        return r;
    };
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        if (k >= a.ncell) continue;  // (no barrier inside the loop)
        const LtmCell cell = ltm_cell<D>(k, npt);
        const int i1 = cell.i1, i2 = cell.i2, i3 = cell.i3;
        int nocc = 0, nemp = 0;
        double dmin = INFINITY, dmax = -INFINITY;
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            int j1 = i1, j2 = i2, j3 = i3;
            ltm_wrap<D>(j1, j2, j3, j, npt);
            const int64_t off = ((int64_t)j3 * npt + j2) * tileE + j1;
            const double ev = Evb[off], ec = Ecb[off], dl = ec - ev;
            nocc += ev <= EF ? 1 : 0;
            nemp += ec > EF ? 1 : 0;
            dmin = fmin(dmin, dl);
            dmax = fmax(dmax, dl);
        }
        if (nocc == 0 || nemp == 0) continue;
        const int i0 = ltm_first(Esl, nE, a.inv_step, dmin);
        if (i0 >= nE) continue;  // every energy lies below the cell
        if (nocc == NV && nemp == NV && !(Esl[i0] < dmax)) {
            // an uncut cell without an energy inside its window: all simplices step at the same index, in one add from the cell's
            // corners (LtmElems::below_add of kernels_ltm.hip: corner 0 and corner (1..1) belong to all d! simplices)
            if constexpr (STATES) {
                LtmVec<NC> m{};
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const bool ends = j == 0 || j == NV - 1;
                    const double wj = D == 3 ? (ends ? 1.5 : 0.5) : (D == 2 ? (ends ? 2.0 / 3.0 : 1.0 / 3.0) : 0.5);
                    const OccVert<NC> cj = cornerV(i1, i2, i3, j);
#pragma unroll
                    for (int cc = 0; cc < NC; ++cc) m.v[cc] += wj * cj.A.v[cc];
                }
#pragma unroll
                for (int cc = 0; cc < NC; ++cc) ltm_add(step + (size_t)cc * nE + i0, m.v[cc]);
            }
            continue;
        }
#pragma unroll 1
        for (int t = 0; t < NS; ++t) {
            OccVert<NC> v[D + 1];
            v[0] = cornerV(i1, i2, i3, 0);
            v[D] = cornerV(i1, i2, i3, NV - 1);
            if constexpr (D == 3) {
                // the permutation (X, Y, Z) of the axes: corners 0, e_X, e_X + e_Y, (1,1,1)
                const int X = t >> 1, Y = (X + 1 + (t & 1)) % 3;
                v[1] = cornerV(i1, i2, i3, 1 << X);
                v[2] = cornerV(i1, i2, i3, (1 << X) | (1 << Y));
            } else if constexpr (D == 2) {
                v[1] = cornerV(i1, i2, i3, 1 << t);
            }
            occ_simplex<D, STATES, NC>(v, EF, Esl, nE, i0, hist, step);
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = lds_occ + nE;
    for (int t = threadIdx.x; t < NC * nE; t += 256) {
        const size_t w = (size_t)NC * nE;  // from one wave's histograms to the next
        partial[(int64_t)t * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
        if (STATES) partial[((int64_t)NC * nE + t) * nrows + prow] = (h[4 * w + t] + h[5 * w + t]) + (h[6 * w + t] + h[7 * w + t]);
    }
}

using LtmOccFn = void (*)(abz_ctx*, dim3, size_t, const LtmOccArgs&, double*, int64_t);
template <int D, bool STATES, int NC>
void ltm_pairs_occ(abz_ctx* ctx, dim3 grid, size_t lds, const LtmOccArgs& a, double* partial, int64_t nrows) {
    launch(ctx, (ltm_pairs_occ_kernel<D, STATES, NC>), grid, dim3(256), (unsigned)lds, a, partial, nrows);
}

// the compiled kernels: [d - 1][states][group: 1, 2, 4 components]
constexpr LtmOccFn LTM_OCC[3][2][3] = {
    {{ltm_pairs_occ<1, false, 1>, ltm_pairs_occ<1, false, 2>, ltm_pairs_occ<1, false, 4>},
     {ltm_pairs_occ<1, true, 1>, ltm_pairs_occ<1, true, 2>, ltm_pairs_occ<1, true, 4>}},
    {{ltm_pairs_occ<2, false, 1>, ltm_pairs_occ<2, false, 2>, ltm_pairs_occ<2, false, 4>},
     {ltm_pairs_occ<2, true, 1>, ltm_pairs_occ<2, true, 2>, ltm_pairs_occ<2, true, 4>}},
    {{ltm_pairs_occ<3, false, 1>, ltm_pairs_occ<3, false, 2>, ltm_pairs_occ<3, false, 4>},
     {ltm_pairs_occ<3, true, 1>, ltm_pairs_occ<3, true, 2>, ltm_pairs_occ<3, true, 4>}},
};

}  // namespace

// The launches of ltm_scan (kernels_ltm.hip) around the occupied kernel: groups of 4, 2, 1 components, chunks of energies.
int launch_ltm_pairs_occupied(abz_ctx* ctx, int d, int npt, PlaneView Esrc, const PlaneView* A, int ncomp, int nb, int v0, int c0, int pnc,
                              double E_F, const double* Es_host, int nE, bool states, double* out_host) {
    if (d < 1 || d > 3 || nb < 1 || pnc < 1 || nb % pnc != 0 || ncomp < 1 || (!A && ncomp != 1)) {
        set_error("launch_ltm_pairs_occupied: d = %d, %d pseudo-bands in rows of %d, %d components%s", d, nb, pnc, ncomp, A ? "" : " of ones");
        return ABZ_ERR_INTERNAL;
    }
    LtmOccArgs a;
    a.E = Esrc;
    a.A = A ? *A : PlaneView{};
    a.acomp = A ? (int64_t)nb * A->pitch : 0;
    a.npt = npt;
    a.ncell = 1;
    for (int j = 0; j < d; ++j) a.ncell *= npt;
    a.v0 = v0;
    a.c0 = c0;
    a.pnc = pnc;
    a.EF = E_F;
    const double weight = 1.0 / ((double)ltm_nsimplex(d) * (double)a.ncell);
    const int ncol = states ? 2 : 1;
    // energies per launch of NC components: the histograms of ltm_window_kernel, the same chunks
    auto chunk = [&](int nc) {
        const size_t fit = (LTM_LDS_MAX - sizeof(uint32_t) * (256 + 8)) / (sizeof(double) * (size_t)(1 + 4 * nc * ncol));
        return (int)std::min<size_t>(fit, states ? 512 : 1024);
    };
    const int64_t nblocks = std::min<int64_t>(cdiv64(a.ncell, 256), std::max(64, std::min(2048, 8192 / nb)));
    const int64_t nrows = nblocks * nb;
    size_t pmax = 0;
    for (int nc : {1, 2, 4})
        if (nc <= ncomp) pmax = std::max(pmax, (size_t)std::min(nE, chunk(nc)) * (size_t)(nc * ncol));
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nrows * pmax);
    if (rc) return rc;
    double* partial = ctx->scratch[1].as<double>();
    EnergyList el;
    // behind the energies: the column sums of a launch, [nc][cnt] sums | [nc][cnt] steps (states)
    if ((rc = energies_to_device(ctx, Es_host, nE, true, 2 * 4 * (size_t)512, el, ncomp))) return rc;
    double* col = el.extra;
    a.inv_step = el.inv_step;
    const dim3 grid((unsigned)nblocks, (unsigned)nb);
    for (int c0g = 0; c0g < ncomp;) {
        const int nc = ncomp - c0g >= 4 ? 4 : (ncomp - c0g >= 2 ? 2 : 1);
        const int CH = chunk(nc);
        const LtmOccFn fn = LTM_OCC[d - 1][states ? 1 : 0][nc == 4 ? 2 : nc - 1];
        a.aplane0 = c0g * nb;
        for (int s0 = 0; s0 < nE; s0 += CH) {
            const int cnt = std::min(CH, nE - s0);
            a.Es = el.dev + s0;
            a.nE = cnt;
            ProfScope ps(ctx, ABZ_K_LTM);
            const size_t lds = sizeof(double) * (size_t)(1 + 4 * nc * ncol) * (size_t)cnt;
            double* const o = el.out + (size_t)c0g * nE + s0;  // results [ncomp][nE] in sorted order
            fn(ctx, grid, lds, a, partial, nrows);
            ABZ_HIP(hipGetLastError());
            if (states) {
                if ((rc = launch_ltm_final(ctx, partial, nrows, 1.0, 2 * nc * cnt, 2 * nc * cnt, 0, col))) return rc;
                if ((rc = launch_ltm_prefix(ctx, col, cnt, nc, weight, (int64_t)nE, o))) return rc;
            } else if ((rc = launch_ltm_final(ctx, partial, nrows, weight, nc * cnt, cnt, nE, o))) {
                return rc;
            }
        }
        c0g += nc;
    }
    return energies_deliver(ctx, el, out_host);
}

}  // namespace abz
