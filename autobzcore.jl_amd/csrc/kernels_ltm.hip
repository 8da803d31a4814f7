// Linear tetrahedron method (gfx950 only): DOS g(E) and state count N(E) from the cached eigenvalues of a full grid.
//
// Bloechl, Jepsen, Andersen, PRB 49, 16223 (1994); the curvature correction (eq. 22) is a mode of the weighted state sum,
// see "Curvature correction" below.  The reference has no counterpart: src/dos_algorithms.jl:1-7 names "LTM" as planned.
//
//  * Geometry.  The grid is periodic; cell (i_1..i_d) has the corners i + {0,1}^d, indices wrapped mod npt, and is
//    cut into d! simplices by the Kuhn (Freudenthal) split: one simplex per permutation of the axes, each walking
//    from corner 0 to corner (1,...,1).  Corner c of a cell is numbered by its bits (bit j: +1 along variable j+1), so
//    the 6 tetrahedra are (0, a, b, 7) with (a, b) = (1,3) (1,5) (2,3) (2,6) (4,5) (4,6), the 2 triangles (0,1,3)
//    (0,2,3).  Every simplex weighs 1 / (d! npt^d); band b of a simplex is the b-th ascending eigenvalue at each
//    corner (no band unfolding).
//  * Formulas.  Sorted corner energies e1 <= ... <= e_{d+1}, e_ij = e_i - e_j, half-open regions e_i <= E < e_{i+1}:
//    the selected region has a positive width, so no selected formula divides by zero; a flat simplex gives 0 to g
//    and a unit step to N.
//      d = 3, g: 3 (E-e1)^2 / (e21 e31 e41) | [3 e21 + 6 x - 3 (e31+e42) x^2 / (e32 e42)] / (e31 e41), x = E-e2 |
//                3 (e4-E)^2 / (e41 e42 e43)
//             N: (E-e1)^3 / (e21 e31 e41) | [e21^2 + 3 e21 x + 3 x^2 - (e31+e42) x^3 / (e32 e42)] / (e31 e41) |
//                1 - (e4-E)^3 / (e41 e42 e43) | 1
//      d = 2, g: 2 (E-e1) / (e21 e31) | 2 (e3-E) / (e31 e32);   N: (E-e1)^2 / (e21 e31) | 1 - (e3-E)^2 / (e31 e32) | 1
//      d = 1, g: 1 / e21;   N: (E-e1) / e21 | 1
//  * Shape (ltm_window_kernel<D, STATES, SLAB, P>, ONE kernel for every scan; P is the payload, see below): that of
//    ggr_window_kernel (kernels_ggr.hip).  The energies are ascending and live in LDS; blockIdx.y is the
//    band, a block walks 256 cells at a time in two passes.  Pass 1, one cell per thread: load the 2^d corner
//    eigenvalues (the i_1 neighbour is the same padded row shifted by one, the i_2 / i_3 neighbours are other lines),
//    find the first energy of the cell's window [min, max) -- by arithmetic in an equispaced list, by binary search
//    otherwise -- and drop the cell when the window holds no energy, as most cells of a coarse sweep do; the others are
//    queued in LDS in thread order (ballot + popcount, no atomics).  Pass 2, one (queued cell, simplex) per thread: sort
//    the simplex (5-compare network), form the reciprocals once and walk the energies inside [e1, e_max).  Without
//    the queue a wave walks the d! simplices of its own 64 cells whenever ONE of them holds an energy, i.e. always,
//    with a fifth of its lanes at work (measured: section 4e of DESIGN).  Sums go into one histogram per wave
//    (workgroup-scope LDS f64 atomics; a wave's own adds come in program order), the histograms of a block are summed
//    in a fixed order into transposed partials, and a fixed-order reduction finishes.  The common weight is applied at
//    the very end.
//  * State count.  A simplex wholly below E counts fully for EVERY higher energy; instead of walking them it adds 1 at
//    the first energy index >= its e_max into a second "step" histogram, which becomes a prefix sum over the sorted
//    energies in the final kernels.  The steps are small integers in f64: their sums are exact in any order, so
//    N(above all bands) = d! npt^d n * weight = n to one rounding, and N(below all bands) is exactly 0.
//  * Locals are plain scalars and fully unrolled constant-index arrays: nothing goes to scratch (DESIGN section 4e has
//    the compiler's resource report).
//  * Payloads.  What a corner carries besides its energy is a policy of the kernel: LtmPlain (nothing; the closed forms above
//    with their fmin / fmax sorting network; a different instruction stream on purpose, 1933 instructions against 2553) or
//    LtmElems<NC, CORR> (NC matrix elements, next item).  The policy gives the per-corner load, picks the simplex routine and
//    says what a cell without an energy in its window adds to the step histogram; the cell walk, the corner geometry (whole
//    grid or slab with its halo plane), the window, the queue and the write-out are the kernel's and exist once.  One final
//    and one prefix kernel serve both (the plain scan is one component), one host function (ltm_scan) launches them, and the
//    table LTM_WINDOWS lists the compiled instantiations: a scan that is not in it is refused.
//  * Matrix elements (LtmElems<NC, false>).  With a quantity A_b(k) per node and band, interpolated linearly inside a
//    simplex like the energy, the same scan gives g_A(E) = sum_b int A_b delta(E - e_b) and N_A(E) = sum_b int A_b
//    theta(E - e_b).  The compare-exchange network that sorts the corner energies swaps the corners' A values along; per
//    (simplex, energy) the d + 1 corner weights w_c are formed from the energies alone and every component adds
//    sum_c w_c A_c.  With t_ij = (E - e_i) / (e_j - e_i), s_j = (e_last - E) / (e_last - e_j), unit = one simplex:
//      d = 3, e1 <= E < e2: q = t12 t13 t14 / 4, N: w_j = q t_1j, w_1 = 4 q - sum;  g: q = t13 t14 / e21, w_j = q t_1j,
//             w_1 = 3 q - sum
//             e2 <= E < e3: the part below E is a prism cut into the tetrahedra (1, P13, P14, 2) (P13, P14, 2, P23)
//             (P14, 2, P23, P24) of volumes v1 = t13 t14, v2 = t14 t23 (1 - t13), v3 = (1 - t14) t23 t24, each giving
//             a quarter of its volume to its vertices; the cut is the triangles (P13, P14, P23) (P14, P23, P24) with
//             densities 3 t13 (1 - t23) / e41 and 3 t23 (1 - t24) / e41, each giving a third to its vertices; a vertex
//             P_ij hands (1 - t_ij, t_ij) of its share to the corners i, j
//             e3 <= E < e4: the mirror image of the first region from corner 4, N: w = 1/4 - (that)
//      d = 2, d = 1: the same with one and two corners fewer (the LtmVec overloads of ltm_simplex2, ltm_simplex1)
//    A simplex wholly below E adds the mean of its corners' A to the step histogram, which is therefore no longer
//    integer; its prefix sum keeps a fixed order.  The elements live in ncomp n planes tiled like the eigenvalue
//    planes (plane c n + b: component c of band b); a launch carries 1, 2 or 4 components, so that the corners of a
//    cell (8 energies + 8 NC elements) stay in registers, and a call walks the grid once per group of components.
//  * Curvature correction (LtmElems<NC, true> with STATES, ABZ_LTM_STATES_CORRECTED).  Linear interpolation misplaces
//    the weight inside a simplex by the band's curvature; to leading order (eq. 22 of the paper for d = 3)
//      N_A^corr(E) = N_A(E) + w sum_T g_T(E) kappa_T,   kappa_T = f_d sum_i A_i (sum_l e_l - (d+1) e_i),   f_d = 1 / (2 (d+1)(d+2)),
//    f_3 = 1/40, f_2 = 1/24, f_1 = 1/12; g_T is the simplex's own DOS, unit = one simplex: the g formulas above.  Window:
//    only a simplex with e_1 <= E < e_{d+1} contributes, the half-open regions of N_A itself, so nothing divides by zero; a
//    flat simplex and one wholly below E give nothing, and the step histogram and pass 1's shortcut are those of N_A.
//    kappa_T is formed once per simplex and component after the sort, g_T per energy from the reciprocals at hand
//    (d = 3: 3 t13 t14 / e21 | 3 [t13 (1 - t23) + t23 (1 - t24)] / e41 | 3 s1 s2 / e43), and g_T kappa_T joins the value that
//    goes into the histogram: no new histogram, launch or atomic.  For A = 1 kappa_T = 0: the state count and the Fermi
//    level have no correction.  The correction removes the leading O(1/npt^2) error of a sum taken at FIXED FILLING, at the
//    Fermi level of the same grid; at a fixed energy the misplaced Fermi surface leaves an error of that order.
//  * Symmetric zones (abz_rule_ltm_unfold).  The scans always walk the whole grid; the eigenvalues they read are invariant
//    under the zone's symmetries, e_b(S k) = e_b(k), so a full-grid rule's planes can be a gather from the irreducible
//    nodes of another rule.  ltm_rank_kernel scatters the node numbers into a table over the grid, ltm_orbit_kernel finds
//    for every grid point the node among its images (the orbit map, 4 B per point, kept by the rule), ltm_unfold_kernel
//    copies: one wave per 64 columns of a padded line, 512 contiguous bytes per plane and store instruction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <type_traits>
#include <vector>

#include "abz_internal.h"
#include "rows_device.h"
#include "sym_image.h"

namespace abz {

namespace {

inline int64_t cdiv64(int64_t a, int64_t b) { return (a + b - 1) / b; }

struct LtmArgs {
    PlaneView E;
    const double* Es;  // device, ascending
    int64_t ncell;     // npt^d
    int npt, nE;
    double inv_step = 0.0;  // > 0: the energies are equispaced: Es[i] = Es[0] + i / inv_step to rounding
};

// A slab of the outermost variable (abz_rule_ltm_halo): E holds the slab's nz planes, `haloE` the one plane behind them
// (plane outer_end mod npt of the grid, a rule of its own); ncell = nz npt^(d-1) and npt stays the grid's.
struct LtmSlabArgs : LtmArgs {
    PlaneView haloE;
    int nz = 0;
};

// first index i with Es[i] >= x (nE if none)
__device__ __forceinline__ int ltm_first(const double* Esl, int nE, double inv_step, double x) {
    int i0 = 0;
    if (inv_step > 0.0) {
        // the index by arithmetic, made exact against the list itself
        const double g = (x - Esl[0]) * inv_step;
        i0 = g <= 0.0 ? 0 : (g >= (double)nE ? nE : (int)g);
        while (i0 > 0 && Esl[i0 - 1] >= x) --i0;
        while (i0 < nE && Esl[i0] < x) ++i0;
    } else {
        int len = nE;
        while (len > 0) {
            const int half = len >> 1;
            const bool right = Esl[i0 + half] < x;
            i0 = right ? i0 + half + 1 : i0;
            len = right ? len - half - 1 : half;
        }
    }
    return i0;
}

__device__ __forceinline__ void ltm_add(double* h, double f) {
    __hip_atomic_fetch_add(h, f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// What a corner of the plain scan carries besides its energy.  The simplex routines of both payloads (LtmPlain, LtmElems
// below) take the corners' payloads behind the energies, so that the scan's one call finds its routine by their type.
struct LtmNone {};

// One tetrahedron with corner energies (a, b, c, d) in any order; i0 = first energy >= the cell's minimum.
template <bool STATES, class P>
__device__ __forceinline__ void ltm_simplex3(double a, double b, double c, double d, LtmNone, LtmNone, LtmNone, LtmNone, const double* Esl,
                                             int nE, int i0, double* hist, double* step) {
    // 5-compare sorting network
    const double lo1 = fmin(a, b), hi1 = fmax(a, b), lo2 = fmin(c, d), hi2 = fmax(c, d);
    const double e1 = fmin(lo1, lo2), m1 = fmax(lo1, lo2), e4 = fmax(hi1, hi2), m2 = fmin(hi1, hi2);
    const double e2 = fmin(m1, m2), e3 = fmax(m1, m2);
    int i = i0;
    if (i < nE && Esl[i] < e4) {
        const double e21 = e2 - e1, e31 = e3 - e1, e41 = e4 - e1, e32 = e3 - e2, e42 = e4 - e2, e43 = e4 - e3;
        // an unselected region may have zero width: its reciprocal is then inf and never read
        const double r1 = 1.0 / (e21 * e31 * e41), r2 = 1.0 / (e31 * e41), q2 = (e31 + e42) / (e32 * e42),
                     r3 = 1.0 / (e41 * e42 * e43);
        for (; i < nE; ++i) {
            const double En = Esl[i];
            if (!(En < e4)) break;
            if (En >= e1) {
                double f;
                if (En < e2) {
                    const double t = En - e1;
                    f = STATES ? t * t * t * r1 : 3.0 * t * t * r1;
                } else if (En < e3) {
                    const double x = En - e2;
                    f = STATES ? (e21 * e21 + 3.0 * e21 * x + 3.0 * x * x - q2 * x * x * x) * r2
                               : (3.0 * e21 + 6.0 * x - 3.0 * q2 * x * x) * r2;
                } else {
                    const double t = e4 - En;
                    f = STATES ? 1.0 - t * t * t * r3 : 3.0 * t * t * r3;
                }
                if (f != 0.0) ltm_add(hist + i, f);
            }
        }
    }
    if (STATES && i < nE) ltm_add(step + i, 1.0);  // i: first energy >= e4
}

template <bool STATES, class P>
__device__ __forceinline__ void ltm_simplex2(double a, double b, double c, LtmNone, LtmNone, LtmNone, const double* Esl, int nE, int i0,
                                             double* hist, double* step) {
    const double lo = fmin(a, b), hi = fmax(a, b);
    const double e1 = fmin(lo, c), e3 = fmax(hi, c), e2 = fmax(lo, fmin(hi, c));
    int i = i0;
    if (i < nE && Esl[i] < e3) {
        const double e21 = e2 - e1, e31 = e3 - e1, e32 = e3 - e2;
        const double r1 = 1.0 / (e21 * e31), r2 = 1.0 / (e31 * e32);
        for (; i < nE; ++i) {
            const double En = Esl[i];
            if (!(En < e3)) break;
            if (En >= e1) {
                double f;
                if (En < e2) {
                    const double t = En - e1;
                    f = STATES ? t * t * r1 : 2.0 * t * r1;
                } else {
                    const double t = e3 - En;
                    f = STATES ? 1.0 - t * t * r2 : 2.0 * t * r2;
                }
                if (f != 0.0) ltm_add(hist + i, f);
            }
        }
    }
    if (STATES && i < nE) ltm_add(step + i, 1.0);
}

template <bool STATES, class P>
__device__ __forceinline__ void ltm_simplex1(double a, double b, LtmNone, LtmNone, const double* Esl, int nE, int i0, double* hist,
                                             double* step) {
    const double e1 = fmin(a, b), e2 = fmax(a, b);
    int i = i0;
    if (i < nE && Esl[i] < e2) {
        const double r1 = 1.0 / (e2 - e1);
        for (; i < nE; ++i) {
            const double En = Esl[i];
            if (!(En < e2)) break;
            if (En >= e1) {
                const double f = STATES ? (En - e1) * r1 : r1;
                if (f != 0.0) ltm_add(hist + i, f);
            }
        }
    }
    if (STATES && i < nE) ltm_add(step + i, 1.0);
}

// ---------------------------------------------------------------------------------------------------------------------
// Matrix elements: g_A(E), N_A(E)
// ---------------------------------------------------------------------------------------------------------------------
struct WLtmArgs {
    PlaneView E, A;
    const double* Es;  // device, ascending
    int64_t ncell;     // npt^d
    int64_t acomp;     // doubles from a band's plane of one component to its plane of the next: n * A.pitch
    int npt, nE;
    int aplane0;       // first element plane of this launch: (its first component) * n
    double inv_step = 0.0;
};

// LtmSlabArgs of the weighted scan: the halo's eigenvalue planes and its element planes (tiled alike, strides of their own)
struct WLtmSlabArgs : WLtmArgs {
    PlaneView haloE, haloA;
    int nz = 0;
};

template <int NC>
struct LtmVec {
    double v[NC];
};

// compare-exchange of two corners: the energies, and the elements with them
template <int NC>
__device__ __forceinline__ void ltm_cx(double& ea, double& eb, LtmVec<NC>& Aa, LtmVec<NC>& Ab) {
    const bool sw = eb < ea;
    const double lo = sw ? eb : ea, hi = sw ? ea : eb;
    ea = lo;
    eb = hi;
#pragma unroll
    for (int c = 0; c < NC; ++c) {
        const double x = sw ? Ab.v[c] : Aa.v[c], y = sw ? Aa.v[c] : Ab.v[c];
        Aa.v[c] = x;
        Ab.v[c] = y;
    }
}

// One tetrahedron, corners in any order.  hist / step: [NC][nE] of the wave.  P: LtmElems<NC, CORR> below.
// CORR (with STATES): the curvature correction, g_T(E) kappa_T added to the sum of the selected region.
template <bool STATES, class P>
__device__ __forceinline__ void ltm_simplex3(double e1, double e2, double e3, double e4, LtmVec<P::NC> A1, LtmVec<P::NC> A2, LtmVec<P::NC> A3,
                                              LtmVec<P::NC> A4, const double* Esl, int nE, int i0, double* hist, double* step) {
    constexpr int NC = P::NC;
    constexpr bool CORR = P::CORR;
    ltm_cx(e1, e2, A1, A2);
    ltm_cx(e3, e4, A3, A4);
    ltm_cx(e1, e3, A1, A3);
    ltm_cx(e2, e4, A2, A4);
    ltm_cx(e2, e3, A2, A3);
    int i = i0;
    if (i < nE && Esl[i] < e4) {
        // an unselected region may have zero width: its reciprocal is then inf and never read
        const double r21 = 1.0 / (e2 - e1), r31 = 1.0 / (e3 - e1), r41 = 1.0 / (e4 - e1), r32 = 1.0 / (e3 - e2), r42 = 1.0 / (e4 - e2),
                     r43 = 1.0 / (e4 - e3);
        LtmVec<NC> kap;  // CORR only
        if constexpr (CORR) {
            const double es = (e1 + e2) + (e3 + e4);
            const double d1 = es - 4.0 * e1, d2 = es - 4.0 * e2, d3 = es - 4.0 * e3, d4 = es - 4.0 * e4;
#pragma unroll
            for (int c = 0; c < NC; ++c) kap.v[c] = 0.025 * ((A1.v[c] * d1 + A2.v[c] * d2) + (A3.v[c] * d3 + A4.v[c] * d4));
        }
        for (; i < nE; ++i) {
            const double En = Esl[i];
            if (!(En < e4)) break;
            if (En >= e1) {
                double w1, w2, w3, w4;
                double gT = 0.0;  // CORR only: the simplex's own g(E), unit = one simplex
                if (En < e2) {
                    const double x = En - e1, t2 = x * r21, t3 = x * r31, t4 = x * r41;
                    const double q = STATES ? 0.25 * (t2 * t3 * t4) : t3 * t4 * r21;
                    if constexpr (CORR) gT = 3.0 * (t3 * t4 * r21);
                    w2 = q * t2;
                    w3 = q * t3;
                    w4 = q * t4;
                    w1 = (STATES ? 4.0 : 3.0) * q - (w2 + w3 + w4);
                } else if (En < e3) {
                    const double x1 = En - e1, x2 = En - e2;
                    const double t13 = x1 * r31, t14 = x1 * r41, t23 = x2 * r32, t24 = x2 * r42;
                    // shares of the vertices P13, P14, P23, P24 and of the corners 1, 2 themselves
                    double p13, p14, p23, p24, c1, c2;
                    if (STATES) {
                        const double v1 = 0.25 * (t13 * t14), v2 = 0.25 * (t14 * t23 * (1.0 - t13)), v3 = 0.25 * ((1.0 - t14) * t23 * t24);
                        p13 = v1 + v2;
                        p14 = v1 + v2 + v3;
                        p23 = v2 + v3;
                        p24 = v3;
                        c1 = v1;
                        c2 = p14;
                        if constexpr (CORR) gT = 3.0 * ((t13 * (1.0 - t23) + t23 * (1.0 - t24)) * r41);
                    } else {
                        const double ga = t13 * (1.0 - t23) * r41, gb = t23 * (1.0 - t24) * r41;
                        p13 = ga;
                        p14 = ga + gb;
                        p23 = p14;
                        p24 = gb;
                        c1 = 0.0;
                        c2 = 0.0;
                    }
                    w1 = c1 + p13 * (1.0 - t13) + p14 * (1.0 - t14);
                    w2 = c2 + p23 * (1.0 - t23) + p24 * (1.0 - t24);
                    w3 = p13 * t13 + p23 * t23;
                    w4 = p14 * t14 + p24 * t24;
                } else {
                    const double y = e4 - En, s1 = y * r41, s2 = y * r42, s3 = y * r43;
                    const double q = STATES ? 0.25 * (s1 * s2 * s3) : s1 * s2 * r43;
                    if constexpr (CORR) gT = 3.0 * (s1 * s2 * r43);
                    const double u1 = q * s1, u2 = q * s2, u3 = q * s3, u4 = (STATES ? 4.0 : 3.0) * q - (u1 + u2 + u3);
                    w1 = STATES ? 0.25 - u1 : u1;
                    w2 = STATES ? 0.25 - u2 : u2;
                    w3 = STATES ? 0.25 - u3 : u3;
                    w4 = STATES ? 0.25 - u4 : u4;
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    double f = (w1 * A1.v[c] + w2 * A2.v[c]) + (w3 * A3.v[c] + w4 * A4.v[c]);
                    if constexpr (CORR) f += gT * kap.v[c];
                    if (f != 0.0) ltm_add(hist + (size_t)c * nE + i, f);
                }
            }
        }
    }
    if (STATES && i < nE) {  // i: first energy >= e4
#pragma unroll
        for (int c = 0; c < NC; ++c) ltm_add(step + (size_t)c * nE + i, 0.25 * ((A1.v[c] + A2.v[c]) + (A3.v[c] + A4.v[c])));
    }
}

template <bool STATES, class P>
__device__ __forceinline__ void ltm_simplex2(double e1, double e2, double e3, LtmVec<P::NC> A1, LtmVec<P::NC> A2, LtmVec<P::NC> A3,
                                              const double* Esl, int nE, int i0, double* hist, double* step) {
    constexpr int NC = P::NC;
    constexpr bool CORR = P::CORR;
    ltm_cx(e1, e2, A1, A2);
    ltm_cx(e2, e3, A2, A3);
    ltm_cx(e1, e2, A1, A2);
    constexpr double third = 1.0 / 3.0;
    int i = i0;
    if (i < nE && Esl[i] < e3) {
        const double r21 = 1.0 / (e2 - e1), r31 = 1.0 / (e3 - e1), r32 = 1.0 / (e3 - e2);
        LtmVec<NC> kap;  // CORR only
        if constexpr (CORR) {
            const double es = (e1 + e2) + e3;
            const double d1 = es - 3.0 * e1, d2 = es - 3.0 * e2, d3 = es - 3.0 * e3;
#pragma unroll
            for (int c = 0; c < NC; ++c) kap.v[c] = (1.0 / 24.0) * ((A1.v[c] * d1 + A2.v[c] * d2) + A3.v[c] * d3);
        }
        for (; i < nE; ++i) {
            const double En = Esl[i];
            if (!(En < e3)) break;
            if (En >= e1) {
                double w1, w2, w3;
                double gT = 0.0;  // CORR only
                if (En < e2) {
                    const double x = En - e1, t2 = x * r21, t3 = x * r31;
                    const double q = STATES ? third * (t2 * t3) : t3 * r21;
                    if constexpr (CORR) gT = 2.0 * (t3 * r21);
                    w2 = q * t2;
                    w3 = q * t3;
                    w1 = (STATES ? 3.0 : 2.0) * q - (w2 + w3);
                } else {
                    const double y = e3 - En, s1 = y * r31, s2 = y * r32;
                    const double q = STATES ? third * (s1 * s2) : s1 * r32;
                    if constexpr (CORR) gT = 2.0 * (s1 * r32);
                    const double u1 = q * s1, u2 = q * s2, u3 = (STATES ? 3.0 : 2.0) * q - (u1 + u2);
                    w1 = STATES ? third - u1 : u1;
                    w2 = STATES ? third - u2 : u2;
                    w3 = STATES ? third - u3 : u3;
                }
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    double f = (w1 * A1.v[c] + w2 * A2.v[c]) + w3 * A3.v[c];
                    if constexpr (CORR) f += gT * kap.v[c];
                    if (f != 0.0) ltm_add(hist + (size_t)c * nE + i, f);
                }
            }
        }
    }
    if (STATES && i < nE) {
#pragma unroll
        for (int c = 0; c < NC; ++c) ltm_add(step + (size_t)c * nE + i, third * ((A1.v[c] + A2.v[c]) + A3.v[c]));
    }
}

template <bool STATES, class P>
__device__ __forceinline__ void ltm_simplex1(double e1, double e2, LtmVec<P::NC> A1, LtmVec<P::NC> A2, const double* Esl, int nE, int i0,
                                              double* hist, double* step) {
    constexpr int NC = P::NC;
    constexpr bool CORR = P::CORR;
    ltm_cx(e1, e2, A1, A2);
    int i = i0;
    if (i < nE && Esl[i] < e2) {
        const double r21 = 1.0 / (e2 - e1);
        LtmVec<NC> kap;  // CORR only: g_T = r21 at every energy of the window, folded in here
        if constexpr (CORR) {
#pragma unroll
            for (int c = 0; c < NC; ++c) kap.v[c] = (1.0 / 12.0) * ((A1.v[c] - A2.v[c]) * (e2 - e1)) * r21;
        }
        for (; i < nE; ++i) {
            const double En = Esl[i];
            if (!(En < e2)) break;
            if (En >= e1) {
                const double t = (En - e1) * r21;
                const double w2 = STATES ? 0.5 * t * t : t * r21, w1 = STATES ? t - w2 : r21 - w2;
#pragma unroll
                for (int c = 0; c < NC; ++c) {
                    double f = w1 * A1.v[c] + w2 * A2.v[c];
                    if constexpr (CORR) f += kap.v[c];
                    if (f != 0.0) ltm_add(hist + (size_t)c * nE + i, f);
                }
            }
        }
    }
    if (STATES && i < nE) {
#pragma unroll
        for (int c = 0; c < NC; ++c) ltm_add(step + (size_t)c * nE + i, 0.5 * (A1.v[c] + A2.v[c]));
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// The scan: one kernel, two payloads
// ---------------------------------------------------------------------------------------------------------------------
constexpr int ltm_nsimplex(int d) { return d == 3 ? 6 : (d == 2 ? 2 : 1); }  // simplices per cell

// A payload says what a corner carries besides its energy (Vec; load, where it carries anything), which routine takes a simplex (the overload of
// ltm_simplex1/2/3 for its Vec) and what a cell adds to the step histogram when no energy falls inside its window (below_add
// per corner, below_put once).  Args<SLAB> is its kernel-argument struct, args() that struct from the host's description of a
// launch (the superset, WLtmSlabArgs).  The hooks are inlined before anything else and call nothing of the kernel's: together
// with the kernel's corner lambdas this keeps the instruction streams of the two kernels this one replaced.
//
// The plain payload: nothing but the energy, the closed forms; every simplex of a cell below E steps by 1.
struct LtmPlain {
    static constexpr int NC = 1;  // histograms per wave and kind
    static constexpr bool ELEMS = false, CORR = false;
    template <bool SLAB>
    using Args = std::conditional_t<SLAB, LtmSlabArgs, LtmArgs>;
    using Vec = LtmNone;
    template <bool SLAB>
    static Args<SLAB> args(const WLtmSlabArgs& s) {
        return LtmSlabArgs{{s.E, s.Es, s.ncell, s.npt, s.nE, s.inv_step}, s.haloE, s.nz};  // (whole grid: its LtmArgs part)
    }
    template <int D>
    static __device__ __forceinline__ void below_add(Vec&, int, const Vec&) {}
    template <int D>
    static __device__ __forceinline__ void below_put(double* step, int, int i0, const Vec&) {
        ltm_add(step + i0, (double)ltm_nsimplex(D));  // every simplex of the cell steps by 1
    }
};

// The element payload: NC components per corner, carried through the sort; CORR: the curvature correction.
template <int NC_, bool CORR_>
struct LtmElems {
    static constexpr int NC = NC_;
    static constexpr bool ELEMS = true, CORR = CORR_;
    template <bool SLAB>
    using Args = std::conditional_t<SLAB, WLtmSlabArgs, WLtmArgs>;
    using Vec = LtmVec<NC>;
    template <bool SLAB>
    static Args<SLAB> args(const WLtmSlabArgs& s) {
        return s;  // (whole grid: its WLtmArgs part)
    }
    // the NC components of the corner whose first one lies at p, `acomp` doubles apart
    static __device__ __forceinline__ Vec load(const double* __restrict__ p, int64_t acomp) {
        Vec r;
#pragma unroll
        for (int c = 0; c < NC; ++c) r.v[c] = p[(int64_t)c * acomp];
        return r;
    }
    // By the sum of the simplices' means in one add per component.  Corner 0 and corner (1..1) belong to all d! simplices, every
    // other corner to d! / d of them... d = 3: (6 (A0 + A7) + 2 sum others) / 4, d = 2: (2 (A0 + A3) + A1 + A2) / 3
    template <int D>
    static __device__ __forceinline__ void below_add(Vec& m, int j, const Vec& Aj) {
        const bool ends = j == 0 || j == (1 << D) - 1;
        const double wj = D == 3 ? (ends ? 1.5 : 0.5) : (D == 2 ? (ends ? 2.0 / 3.0 : 1.0 / 3.0) : 0.5);
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) m.v[cc] += wj * Aj.v[cc];
    }
    template <int D>
    static __device__ __forceinline__ void below_put(double* step, int nE, int i0, const Vec& m) {
#pragma unroll
        for (int cc = 0; cc < NC; ++cc) ltm_add(step + (size_t)cc * nE + i0, m.v[cc]);
    }
};

// Passes with at most this many of their 256 cells queued redistribute the simplices over the block; measured on the
// 150^3 grid of 3 bands: 32 energies (a fifth of the cells queued) 0.23 ms direct, 0.14 ms queued; 256 energies (most
// cells queued) 0.28 ms direct, 0.46 ms queued.
constexpr unsigned LTM_QUEUE_MAX = 128;

// partial [(STATES ? 2 : 1) NC nE][nrows]: columns c nE + i the formula sums of component c, NC nE + c nE + i its steps
// SLAB (d >= 2): the cells of a slab of the outermost variable (the `corner` lambda); everything else is as on the whole grid.
// P: LtmPlain or LtmElems<NC, CORR> (CORR with STATES only: N_A with the curvature correction; same histograms, same launches).
template <int D, bool STATES, bool SLAB, class P>
__global__ __launch_bounds__(256) void ltm_window_kernel(typename P::template Args<SLAB> a, double* __restrict__ partial, int64_t nrows) {
    static_assert(!SLAB || D >= 2, "a slab needs at least two variables");
    static_assert(STATES || !P::CORR, "the curvature correction belongs to the state sum");
    // [nE] energies | [4 waves][NC][nE] sums | STATES: [4 waves][NC][nE] steps | [256] queue of a pass | [2][4] per-wave counts
    extern __shared__ __attribute__((aligned(16))) double ldsl[];
    using Vec = typename P::Vec;
    constexpr int NC = P::NC;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nE = a.nE;
    constexpr int NH = (STATES ? 8 : 4) * NC;
    constexpr int NS = ltm_nsimplex(D);
    constexpr int NV = 1 << D;  // corners per cell
    const double* const Esl = ldsl;
    double* const hist = ldsl + (size_t)(1 + wave * NC) * nE;
    double* const step = ldsl + (size_t)(1 + (4 + wave) * NC) * nE;  // STATES only
    uint32_t* const queue = reinterpret_cast<uint32_t*>(ldsl + (size_t)(1 + NH) * nE);
    uint32_t* const wcount = queue + 256;
    for (int i = threadIdx.x; i < nE; i += 256) ldsl[i] = a.Es[i];
    for (int i = threadIdx.x; i < NH * nE; i += 256) ldsl[nE + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    // this band's eigenvalue planes and their line stride; ELEMS: the planes of the launch's first component
    const double* __restrict__ const Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    [[maybe_unused]] const double* __restrict__ Ab = nullptr;
    const int64_t tileE = a.E.tile;
    [[maybe_unused]] int64_t tileA = 0, acomp = 0;
    if constexpr (P::ELEMS) {
        Ab = a.A.base + (int64_t)(a.aplane0 + (int)blockIdx.y) * a.A.pitch;
        tileA = a.A.tile;
        acomp = a.acomp;
    }
    [[maybe_unused]] const double* __restrict__ EHb = nullptr;  // SLAB: this band's planes of the halo, their line strides, the slab's planes
    [[maybe_unused]] const double* __restrict__ AHb = nullptr;
    [[maybe_unused]] int64_t htileE = 0, htileA = 0;
    [[maybe_unused]] int nz = 0;
    if constexpr (SLAB) {
        EHb = a.haloE.base + (int64_t)blockIdx.y * a.haloE.pitch;
        htileE = a.haloE.tile;
        if constexpr (P::ELEMS) {
            AHb = a.haloA.base + (int64_t)(a.aplane0 + (int)blockIdx.y) * a.haloA.pitch;
            htileA = a.haloA.tile;
        }
        nz = a.nz;
    }
    // THE geometry, for energies and elements alike: corner `bits` (bit j: +1 along variable j+1) of cell (i1, i2, i3), which
    // become the corner's own indices.  Whole grid: every index wraps mod npt, the corner is column i1 of line i3 npt + i2 of the
    // band's planes.  SLAB: the outermost index is local to the slab's nz planes and does not wrap; true: the corner lies behind
    // plane nz - 1, in the halo plane, at column i1 of its line i2 (d = 2: of its only line, 0).
    auto corner = [&](int& i1, int& i2, int& i3, int bits) -> bool {
        if ((bits & 1) && ++i1 == npt) i1 = 0;
        if constexpr (SLAB) {
            if constexpr (D == 3) {
                if ((bits & 2) && ++i2 == npt) i2 = 0;
                return (bits & 4) && ++i3 == nz;
            } else {
                if ((bits & 2) && ++i2 == nz) {
                    i2 = 0;
                    return true;
                }
            }
        } else {
            if (D >= 2 && (bits & 2) && ++i2 == npt) i2 = 0;
            if (D == 3 && (bits & 4) && ++i3 == npt) i3 = 0;
        }
        return false;
    };
    auto cornerE = [&](int i1, int i2, int i3, int bits) -> double {
        [[maybe_unused]] const bool halo = corner(i1, i2, i3, bits);
        if constexpr (SLAB) {
            if (halo) return EHb[(int64_t)i2 * htileE + i1];
        }
        return Eb[((int64_t)i3 * npt + i2) * tileE + i1];
    };
    auto cornerA = [&](int i1, int i2, int i3, int bits) -> Vec {
        if constexpr (P::ELEMS) {
            const bool halo = corner(i1, i2, i3, bits);
            return P::load(SLAB && halo ? AHb + (int64_t)i2 * htileA + i1 : Ab + ((int64_t)i3 * npt + i2) * tileA + i1, acomp);
        } else {
            return {};  // the plain scan has no element planes
        }
    };
    // Two passes over 256 cells at a time (the trip count is the block's, so the barriers are uniform).  Pass 1, one cell
    // per thread: the cell's window against the energy list; cells that hold an energy are queued, in thread order.  Pass 2,
    // one (queued cell, simplex) per thread: in a coarse sweep a fifth of the cells holds an energy, and a wave that walked
    // the 6 simplices of its own cells would do so for nearly every cell (some lane always has one) with most lanes idle.
    unsigned pass = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        bool active = false;
        int i0 = 0, i1 = 0, i2 = 0, i3 = 0;
        double c[NV];
        if (k < a.ncell) {
            const int64_t line = k <= 0xffffffffll ? (int64_t)((uint32_t)k / (uint32_t)npt) : k / npt;
            i1 = (int)(k - line * npt);
            i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
            i2 = (int)line - i3 * npt;
#pragma unroll
            for (int j = 0; j < NV; ++j) c[j] = cornerE(i1, i2, i3, j);
            double cmin = c[0], cmax = c[0];
#pragma unroll
            for (int j = 1; j < NV; ++j) {
                cmin = fmin(cmin, c[j]);
                cmax = fmax(cmax, c[j]);
            }
            i0 = ltm_first(Esl, nE, a.inv_step, cmin);
            if (i0 < nE) {  // else every energy lies below the cell
                if (Esl[i0] < cmax) active = true;
                else if (STATES) {
                    // no energy inside the window: all simplices step at the same index, in one add from the cell's corners
                    Vec m{};
#pragma unroll
                    for (int j = 0; j < NV; ++j) P::template below_add<D>(m, j, cornerA(i1, i2, i3, j));
                    P::template below_put<D>(step, nE, i0, m);
                }
            }
        }
        const unsigned long long mask = __ballot(active);
        // the counts alternate between two sets: a direct pass has this one barrier only, and a thread that is already
        // in the next pass must not overwrite the counts a slower one is still reading
        uint32_t* const wc = wcount + 4 * (pass & 1);
        ++pass;
        if (lane == 0) wc[wave] = (uint32_t)__popcll(mask);
        __syncthreads();
        uint32_t off = 0, total = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t cw = wc[w];
            off += w < wave ? cw : 0u;
            total += cw;
        }
        if (total > LTM_QUEUE_MAX) {
            // Most cells hold an energy (a fine sweep): every thread walks the simplices of its own cell from the corner
            // energies it still holds (their elements are loaded now); the queue would only add its reloads.  `total` is
            // the block's: a uniform branch.
            if (active) {
                Vec Av[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) Av[j] = cornerA(i1, i2, i3, j);
                if constexpr (D == 3) {
                    ltm_simplex3<STATES, P>(c[0], c[1], c[3], c[7], Av[0], Av[1], Av[3], Av[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES, P>(c[0], c[1], c[5], c[7], Av[0], Av[1], Av[5], Av[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES, P>(c[0], c[2], c[3], c[7], Av[0], Av[2], Av[3], Av[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES, P>(c[0], c[2], c[6], c[7], Av[0], Av[2], Av[6], Av[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES, P>(c[0], c[4], c[5], c[7], Av[0], Av[4], Av[5], Av[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES, P>(c[0], c[4], c[6], c[7], Av[0], Av[4], Av[6], Av[7], Esl, nE, i0, hist, step);
                } else if constexpr (D == 2) {
                    ltm_simplex2<STATES, P>(c[0], c[1], c[3], Av[0], Av[1], Av[3], Esl, nE, i0, hist, step);
                    ltm_simplex2<STATES, P>(c[0], c[2], c[3], Av[0], Av[2], Av[3], Esl, nE, i0, hist, step);
                } else {
                    ltm_simplex1<STATES, P>(c[0], c[1], Av[0], Av[1], Esl, nE, i0, hist, step);
                }
            }
            continue;
        }
        if (active) queue[off + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = ((uint32_t)i0 << 8) | threadIdx.x;
        __syncthreads();  // the next pass writes the queue after its own first barrier
        for (uint32_t p = threadIdx.x; p < NS * total; p += 256) {
            const uint32_t cell = p / NS, t = p - cell * NS;
            const uint32_t q = queue[cell];
            const int j0 = (int)(q >> 8);
            const int64_t kq = base + (q & 255u);
            const int64_t line = kq <= 0xffffffffll ? (int64_t)((uint32_t)kq / (uint32_t)npt) : kq / npt;
            const int q1 = (int)(kq - line * npt);
            const int q3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
            const int q2 = (int)line - q3 * npt;
            const double c0 = cornerE(q1, q2, q3, 0), c1 = cornerE(q1, q2, q3, NV - 1);
            const Vec A0 = cornerA(q1, q2, q3, 0), A1 = cornerA(q1, q2, q3, NV - 1);
            if constexpr (D == 3) {
                // the permutation (X, Y, Z) of the axes: corners 0, e_X, e_X + e_Y, (1,1,1)
                const int X = (int)(t >> 1), Y = (X + 1 + (int)(t & 1)) % 3;
                const int ba = 1 << X, bb = (1 << X) | (1 << Y);
                ltm_simplex3<STATES, P>(c0, cornerE(q1, q2, q3, ba), cornerE(q1, q2, q3, bb), c1, A0, cornerA(q1, q2, q3, ba),
                                            cornerA(q1, q2, q3, bb), A1, Esl, nE, j0, hist, step);
            } else if constexpr (D == 2) {
                ltm_simplex2<STATES, P>(c0, cornerE(q1, q2, q3, 1 << t), c1, A0, cornerA(q1, q2, q3, 1 << t), A1, Esl, nE, j0, hist, step);
            } else {
                ltm_simplex1<STATES, P>(c0, c1, A0, A1, Esl, nE, j0, hist, step);
            }
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = ldsl + nE;
    // transposed partials [column][row]: the final reduction reads the rows of one column contiguously; column c nE + t
    // sits at the same place in every wave's block
    for (int t = threadIdx.x; t < NC * nE; t += 256) {
        const size_t w = (size_t)NC * nE;  // from one wave's histograms to the next
        partial[(int64_t)t * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
        if (STATES) partial[((int64_t)NC * nE + t) * nrows + prow] = (h[4 * w + t] + h[5 * w + t]) + (h[6 * w + t] + h[7 * w + t]);
    }
}

// out[c * ostride + i] = scale * sum_rows partial[c * cnt + i][row], one block per column (c, i), fixed summation order
// (ggr_final_kernel's)
__global__ __launch_bounds__(256) void ltm_final_kernel(const double* __restrict__ partial, int64_t nrows, double scale, int cnt,
                                                        int64_t ostride, double* __restrict__ out) {
    __shared__ double red[256];
    const double* __restrict__ p = partial + (int64_t)blockIdx.x * nrows;
    double s = 0.0;
    for (int64_t r = threadIdx.x; r < nrows; r += 256) s += p[r];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] += red[threadIdx.x + w];
        __syncthreads();
    }
    const int c = (int)blockIdx.x / cnt, i = (int)blockIdx.x - c * cnt;
    if (threadIdx.x == 0) out[(int64_t)c * ostride + i] = scale * red[0];
}

// State count of a chunk, one block per component: out[c * ostride + i] = weight * (sums[c][i] + steps[c][0] + ... + steps[c][i]);
// col = [nc][nE] sums | [nc][nE] steps, nE <= 512.  The prefix sum runs in index order, the same at every call (the plain
// scan's steps are integers, their sums exact; means of elements are not).
__global__ __launch_bounds__(256) void ltm_prefix_kernel(const double* __restrict__ col, int nE, int nc, double weight, int64_t ostride,
                                                         double* __restrict__ out) {
    __shared__ double st[512];
    const int c = (int)blockIdx.x;
    for (int i = threadIdx.x; i < nE; i += 256) st[i] = col[(size_t)(nc + c) * nE + i];
    __syncthreads();
    for (int i = threadIdx.x; i < nE; i += 256) {
        double run = 0.0;
        for (int j = 0; j <= i; ++j) run += st[j];
        out[(int64_t)c * ostride + i] = weight * (col[(size_t)c * nE + i] + run);
    }
}

// host array of one component [nk][n] -> its n planes: plane0 + b, node k
__global__ __launch_bounds__(256) void ltm_repack_kernel(const double* __restrict__ src, PlaneView A, int plane0, int n, int64_t nk) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= nk * n) return;
    const int64_t k = t / n;
    const int b = (int)(t - k * n);
    const int64_t line = k / A.line_len;
    A.base[line * A.tile + (int64_t)(plane0 + b) * A.pitch + (k - line * A.line_len)] = src[t];
}

// smallest and largest eigenvalue of the n planes (padding excluded): out[2 block + {0, 1}]
__global__ __launch_bounds__(256) void ltm_minmax_kernel(PlaneView E, int n, int64_t nk, double* __restrict__ out) {
    __shared__ double lo[256], hi[256];
    double mn = INFINITY, mx = -INFINITY;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < nk * n; t += (int64_t)gridDim.x * 256) {
        const int64_t b = t / nk, k = t - b * nk;
        const int64_t line = k / E.line_len;
        const double v = E.base[line * E.tile + b * E.pitch + (k - line * E.line_len)];
        mn = fmin(mn, v);
        mx = fmax(mx, v);
    }
    lo[threadIdx.x] = mn;
    hi[threadIdx.x] = mx;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            lo[threadIdx.x] = fmin(lo[threadIdx.x], lo[threadIdx.x + w]);
            hi[threadIdx.x] = fmax(hi[threadIdx.x], hi[threadIdx.x + w]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[2 * blockIdx.x] = lo[0];
        out[2 * blockIdx.x + 1] = hi[0];
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Eigenvalues of the whole grid from those of the irreducible nodes (abz_rule_ltm_unfold): e_b(S k) = e_b(k)
// ---------------------------------------------------------------------------------------------------------------------
// rank[flat index of node k] = k.  idx [d][nk] holds grid indices inside 0 .. npt-1 (device-built lists by construction,
// explicit lists are checked when their rule is built); a list that names a point twice leaves either of the two.
__global__ __launch_bounds__(256) void ltm_rank_kernel(const int32_t* __restrict__ idx, int64_t nk, int d, int npt, int64_t N,
                                                       int32_t* __restrict__ rank) {
    const int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (k >= nk) return;
    int64_t lin = 0, mul = 1;
    for (int j = 0; j < d; ++j) {
        lin += (int64_t)idx[(int64_t)j * nk + k] * mul;
        mul *= npt;
    }
    if (lin >= 0 && lin < N) rank[lin] = (int32_t)k;
}

// One thread per grid point: the node it is, or the node among its images (sym_image: the integer matrices on grid
// indices mod npt) that comes first in the set's order.  Which image of an orbit the list keeps does not matter.
__global__ __launch_bounds__(256) void ltm_orbit_kernel(SymArgs a, const int32_t* __restrict__ rank, int32_t* __restrict__ node_of,
                                                        int* __restrict__ missing) {
    const int64_t lin = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (lin >= a.N) return;
    int32_t k = rank[lin];
    if (k < 0) {
        int v[3] = {0, 0, 0};
        int64_t r = lin;
        for (int j = 0; j < a.d; ++j) {
            v[j] = (int)(r % a.npt);
            r /= a.npt;
        }
        for (int s = 0; s < a.nsyms && k < 0; ++s) {
            const int64_t img = sym_image(a, v, s);  // inside 0 .. N-1: every coordinate is reduced mod npt
            k = rank[img];
        }
        if (k < 0) atomicAdd(missing, 1);
    }
    node_of[lin] = k;
}

// One wave per 64 consecutive columns of a padded grid line: each lane reads its point's node once and copies the n
// eigenvalues of that node (a source of a few MB at most: it stays in L2) into the n planes; the stores of a wave are
// 512 contiguous bytes per plane, the rows the builders write.  Padding columns npt .. row-1 get zeros.
__global__ __launch_bounds__(256) void ltm_unfold_kernel(PlaneView src, PlaneView dst, const int32_t* __restrict__ node_of, int n,
                                                         int npt, int chunks, int64_t nunits) {
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= nunits) return;
    const int64_t line = u / chunks;
    const int i = (int)(u - line * chunks) * 64 + (int)(threadIdx.x & 63);
    if (i >= dst.row) return;
    double* __restrict__ const out = dst.base + line * dst.tile + i;
    const int32_t k = i < npt ? node_of[line * npt + i] : -1;
    if (k < 0) {
        for (int b = 0; b < n; ++b) out[(int64_t)b * dst.pitch] = 0.0;
        return;
    }
    const double* __restrict__ const in = src.base + view_off(src, k);
#pragma unroll 4
    for (int b = 0; b < n; ++b) out[(int64_t)b * dst.pitch] = in[(int64_t)b * src.pitch];
}

// dynamic LDS of the plain g scan at 1024 energies: 5 x 1024 x 8 B + queue and counts; every scan stays within it
constexpr size_t LTM_LDS_MAX = sizeof(double) * 5 * 1024 + sizeof(uint32_t) * (256 + 8);

using LtmWindowFn = void (*)(abz_ctx*, dim3, size_t, const WLtmSlabArgs&, double*, int64_t);
template <int D, bool STATES, bool SLAB, class P>
void ltm_window(abz_ctx* ctx, dim3 grid, size_t lds, const WLtmSlabArgs& a, double* partial, int64_t nrows) {
    launch(ctx, (ltm_window_kernel<D, STATES, SLAB, P>), grid, dim3(256), (unsigned)lds, P::template args<SLAB>(a), partial, nrows);
}

// The compiled window kernels, all of them: a scan that is not in this table is refused.
struct LtmWindowRow {
    int d;
    bool states, slab, elems;
    int nc;
    bool corr;
    LtmWindowFn fn;
};
template <int D, bool STATES, bool SLAB, class P>
constexpr LtmWindowRow ltm_row() {
    return {D, STATES, SLAB, P::ELEMS, P::NC, P::CORR, ltm_window<D, STATES, SLAB, P>};
}
// the element payloads of the table: without and with the curvature correction; the digit is NC
using Elems1 = LtmElems<1, false>;
using Elems2 = LtmElems<2, false>;
using Elems4 = LtmElems<4, false>;
using Corr1 = LtmElems<1, true>;
using Corr2 = LtmElems<2, true>;
using Corr4 = LtmElems<4, true>;
constexpr LtmWindowRow LTM_WINDOWS[] = {
    // plain, whole grid (6) and slab (4)
    ltm_row<1, false, false, LtmPlain>(), ltm_row<2, false, false, LtmPlain>(), ltm_row<3, false, false, LtmPlain>(),
    ltm_row<1, true, false, LtmPlain>(), ltm_row<2, true, false, LtmPlain>(), ltm_row<3, true, false, LtmPlain>(),
    ltm_row<2, false, true, LtmPlain>(), ltm_row<3, false, true, LtmPlain>(),
    ltm_row<2, true, true, LtmPlain>(), ltm_row<3, true, true, LtmPlain>(),
    // elements, whole grid: g_A and N_A with 1, 2, 4 components (18)
    ltm_row<1, false, false, Elems1>(), ltm_row<2, false, false, Elems1>(), ltm_row<3, false, false, Elems1>(),
    ltm_row<1, false, false, Elems2>(), ltm_row<2, false, false, Elems2>(), ltm_row<3, false, false, Elems2>(),
    ltm_row<1, false, false, Elems4>(), ltm_row<2, false, false, Elems4>(), ltm_row<3, false, false, Elems4>(),
    ltm_row<1, true, false, Elems1>(), ltm_row<2, true, false, Elems1>(), ltm_row<3, true, false, Elems1>(),
    ltm_row<1, true, false, Elems2>(), ltm_row<2, true, false, Elems2>(), ltm_row<3, true, false, Elems2>(),
    ltm_row<1, true, false, Elems4>(), ltm_row<2, true, false, Elems4>(), ltm_row<3, true, false, Elems4>(),
    // elements, whole grid: corrected N_A (9)
    ltm_row<1, true, false, Corr1>(), ltm_row<2, true, false, Corr1>(), ltm_row<3, true, false, Corr1>(),
    ltm_row<1, true, false, Corr2>(), ltm_row<2, true, false, Corr2>(), ltm_row<3, true, false, Corr2>(),
    ltm_row<1, true, false, Corr4>(), ltm_row<2, true, false, Corr4>(), ltm_row<3, true, false, Corr4>(),
    // elements, slab: one component (the energy as the element), g_A, N_A, corrected N_A (6)
    ltm_row<2, false, true, Elems1>(), ltm_row<3, false, true, Elems1>(),
    ltm_row<2, true, true, Elems1>(), ltm_row<3, true, true, Elems1>(),
    ltm_row<2, true, true, Corr1>(), ltm_row<3, true, true, Corr1>(),
};
static_assert(sizeof(LTM_WINDOWS) / sizeof(LTM_WINDOWS[0]) == 43, "the shipped window kernels");

LtmWindowFn ltm_window_fn(int d, bool states, bool slab, bool elems, int nc, bool corr) {
    for (const LtmWindowRow& r : LTM_WINDOWS)
        if (r.d == d && r.states == states && r.slab == slab && r.elems == elems && r.nc == nc && r.corr == corr) return r.fn;
    return nullptr;
}

// The scan behind launch_ltm (A == nullptr: the plain payload, one "component") and launch_ltm_weighted.
int ltm_scan(abz_ctx* ctx, const char* who, int n, int d, int npt, PlaneView E, const PlaneView* A, int ncomp, const double* Es_host, int nE,
             int what, double* out_host, const LtmSlab* slab) {
    const bool states = what != ABZ_LTM_DOS, corrected = what == ABZ_LTM_STATES_CORRECTED;
    WLtmSlabArgs a;  // the superset: every kernel takes its own part (args() of its payload)
    a.E = E;
    a.npt = npt;
    a.ncell = 1;
    for (int j = 0; j < d; ++j) a.ncell *= npt;
    if (A) {
        a.A = *A;
        a.acomp = (int64_t)n * A->pitch;
    }
    // the weight of a simplex is the whole grid's: the partial sums of the slabs of a partition add up to the grid's value
    const double weight = 1.0 / ((double)ltm_nsimplex(d) * (double)a.ncell);
    if (slab) {
        if (d < 2 || slab->nz < 1 || slab->nz > npt || !slab->E.base || (A && (!slab->A.base || ncomp != 1))) {
            if (A) set_error("%s: a slab of %d planes of a %d-d grid of %d points with %d components", who, slab->nz, d, npt, ncomp);
            else set_error("%s: a slab of %d planes of a %d-d grid of %d points", who, slab->nz, d, npt);
            return ABZ_ERR_INTERNAL;
        }
        a.haloE = slab->E;
        if (A) a.haloA = slab->A;
        a.nz = slab->nz;
        a.ncell = a.ncell / npt * slab->nz;
    }
    // the window kernels of the component groups this call will form (4s, then a 2, then a 1): refused before anything is
    // reserved or launched
    LtmWindowFn window[5] = {};
    for (int nc : {1, 2, 4}) {
        if (!(nc == 4 ? ncomp >= 4 : (ncomp % 4 & nc) != 0)) continue;
        window[nc] = ltm_window_fn(d, states, slab != nullptr, A != nullptr, nc, corrected);
        if (!window[nc]) {
            set_error("%s: no tetrahedron scan for d = %d, what = %d, %d components%s%s", who, d, what, nc, A ? " of elements" : "",
                      slab ? ", on a slab" : "");
            return ABZ_ERR_INTERNAL;
        }
    }
    const int ncol = states ? 2 : 1;
    // Energies per launch of NC components: 8 (1 + 4 NC ncol) B of LDS each (+ 1 KB of queue), within LTM_LDS_MAX, and at most
    // 512 where the prefix kernel holds a chunk's steps: g 1024 / 568 / 301, N 512 / 301 / 155 for NC = 1 / 2 / 4.  Chunks are
    // independent: the steps of all simplices below a chunk's first energy land on its index 0.
    auto chunk = [&](int nc) {
        const size_t fit = (LTM_LDS_MAX - sizeof(uint32_t) * (256 + 8)) / (sizeof(double) * (size_t)(1 + 4 * nc * ncol));
        return (int)std::min<size_t>(fit, states ? 512 : 1024);
    };
    // one block row per band; enough blocks to fill the device several times over, few enough partial rows to sum
    const int64_t nblocks = std::min<int64_t>(cdiv64(a.ncell, 256), std::max(64, std::min(2048, 8192 / n)));
    const int64_t nrows = nblocks * n;
    size_t pmax = 0;
    for (int nc : {1, 2, 4})
        if (nc <= ncomp) pmax = std::max(pmax, (size_t)std::min(nE, chunk(nc)) * (size_t)(nc * ncol));
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nrows * pmax);
    if (rc) return rc;
    double* partial = ctx->scratch[1].as<double>();
    EnergyList el;
    // behind the energies: the column sums of a launch, [nc][cnt] sums | [nc][cnt] steps (states)
    if ((rc = energies_to_device(ctx, Es_host, nE, true, A ? 2 * 4 * (size_t)512 : 2 * (size_t)chunk(1), el, ncomp))) return rc;
    double* col = el.extra;
    a.inv_step = el.inv_step;
    const dim3 grid((unsigned)nblocks, (unsigned)n);
    // groups of 4 components, then 2, then 1; every group walks the grid once per chunk of energies
    for (int c0 = 0; c0 < ncomp;) {
        const int nc = ncomp - c0 >= 4 ? 4 : (ncomp - c0 >= 2 ? 2 : 1);
        const int CH = chunk(nc);
        a.aplane0 = c0 * n;
        for (int s0 = 0; s0 < nE; s0 += CH) {
            const int cnt = std::min(CH, nE - s0);
            a.Es = el.dev + s0;
            a.nE = cnt;
            ProfScope ps(ctx, ABZ_K_LTM);
            const size_t lds = sizeof(double) * (size_t)(1 + 4 * nc * ncol) * (size_t)cnt + sizeof(uint32_t) * (256 + 8);
            double* const o = el.out + (size_t)c0 * nE + s0;  // results [ncomp][nE] in sorted order
            window[nc](ctx, grid, lds, a, partial, nrows);
            ABZ_HIP(hipGetLastError());
            if (states) {
                launch(ctx, ltm_final_kernel, dim3((unsigned)(2 * nc * cnt)), dim3(256), 0, partial, nrows, 1.0, 2 * nc * cnt, (int64_t)0, col);
                ABZ_HIP(hipGetLastError());
                launch(ctx, ltm_prefix_kernel, dim3((unsigned)nc), dim3(256), 0, col, cnt, nc, weight, (int64_t)nE, o);
            } else {
                launch(ctx, ltm_final_kernel, dim3((unsigned)(nc * cnt)), dim3(256), 0, partial, nrows, weight, cnt, (int64_t)nE, o);
            }
            ABZ_HIP(hipGetLastError());
        }
        c0 += nc;
    }
    return energies_deliver(ctx, el, out_host);
}

// ---------------------------------------------------------------------------------------------------------------------
// Trace of the Green's function at complex energies (abz_rule_ltm_green)
// ---------------------------------------------------------------------------------------------------------------------
// tr G(z) = w sum_{cells} sum_{d! simplices} sum_{bands} J[x_0 .. x_d](z), w = 1 / (d! npt^d), on the mesh of the scans above.
// J[x_0 .. x_m](z) is the mean of 1 / (z - e) over a simplex in which e is linear with the sorted corner values x_0 <= .. <= x_m
// (the mean over the normalised B-spline with those knots).  With u_i = z - x_i, which all share Im z > 0:
//      m = 0:  J = 1 / u_0
//      m = 1:  J = (log u_0 - log u_1) / (x_1 - x_0)     principal logs of one open half plane: no branch fix-up
//      m >= 2: J[x_0..x_m] = m / (m-1) (u_0 J[x_0..x_{m-1}] - u_m J[x_1..x_m]) / (x_m - x_0)
//  * Evaluation rule.  The recursion divides by a width and loses |u| / width per level; a symmetric grid is full of equal and
//    nearly equal corners.  A sub-range x_i..x_j with x_j - x_i < rho |z - mean|, rho = 1/2, is summed by its Taylor series
//      J = sum_k  m! k! / (m+k)!  h_k(delta) / ubar^(k+1),   delta_l = x_l - mean,  ubar = z - mean,
//    h_k the complete homogeneous symmetric polynomial by H_l^(k) = H_(l-1)^(k) + delta_l H_l^(k-1), H_0^(k) = delta_0^k: one
//    row of m + 1 registers carried from k - 1 to k, the coefficients from a table.  It stops when (max |delta| / |ubar|)^k < 2^-52:
//    max |delta| <= m / (m+1) width, so the ratio stays below 3/8 and 37 terms are the most a sub-range takes.  Only wider
//    sub-ranges recurse: nothing is divided by a width below rho |ubar|.  The series runs on delta / |ubar| and ubar / |ubar|, so
//    neither power leaves the range of a double; at width 0 it is 1 / u.
//  * Shape (ltm_green_kernel<D>).  Not a window scan: every simplex contributes at every z, there is no queue and no histogram.
//    The cell walk and the whole-grid corner geometry are ltm_window_kernel's: blocks of 256 cells, one cell per thread,
//    blockIdx.y the band, the 2^d corner energies in registers, the values of z in LDS.  Per (cell, z) the 2^d complex logs of
//    z - e_corner are taken once and shared by the cell's d! simplices; the sorting network of a simplex carries each corner's
//    log along with its energy, as LtmElems carries elements, and the pair formula reads them.  blockIdx.z splits the values of
//    z of a launch where the cells alone do not fill the device.
//  * Reduction.  Per z in a fixed order: a butterfly over the wave, lane 0 adds into the wave's LDS slot [nz][re, im] in
//    program order, the four waves are summed as above into transposed partials and ltm_final_kernel finishes.  No atomics:
//    two calls return the same bits.
constexpr double GREEN_RHO2 = 0.25;      // rho^2
constexpr double GREEN_EPS2 = 0x1p-104;  // (2^-52)^2
constexpr int GREEN_KMAX = 40;           // terms beyond k = 37 (the five knots of a corner weight: 39) are never asked for
constexpr int LTM_GREEN_CHUNK = 512;     // values of z per launch: 8 (2 + 4 x 2) B of LDS each
static_assert(sizeof(double) * 10 * LTM_GREEN_CHUNK <= LTM_LDS_MAX, "the z list and the four waves' sums fit the scans' LDS");

// m! k! / (m+k)! for m = 1, 2, 3 and, for the five knots of a corner weight in 3-D, 4
struct GreenCoef {
    double c[4][GREEN_KMAX + 1];
};
constexpr GreenCoef green_coef() {
    GreenCoef t{};
    for (int m = 1; m <= 4; ++m) {
        t.c[m - 1][0] = 1.0;
        for (int k = 1; k <= GREEN_KMAX; ++k) t.c[m - 1][k] = t.c[m - 1][k - 1] * (double)k / (double)(m + k);
    }
    return t;
}
__constant__ const GreenCoef GREEN_COEF = green_coef();

struct GreenArgs {
    PlaneView E;
    const double* z;  // device [nz][2]: re, im > 0
    int64_t ncell;    // npt^d
    int npt, nz;
    int zper;         // values of z per blockIdx.z
};

struct Cx {
    double re, im;
};
__device__ __forceinline__ Cx cx_mul(Cx a, Cx b) { return {a.re * b.re - a.im * b.im, a.re * b.im + a.im * b.re}; }

// what the sort of a simplex carries per corner: the energy and log(z - energy)
struct GreenCorner {
    double x, lr, li;
};
__device__ __forceinline__ GreenCorner green_sel(bool first, const GreenCorner& a, const GreenCorner& b) {
    return {first ? a.x : b.x, first ? a.lr : b.lr, first ? a.li : b.li};
}
__device__ __forceinline__ void green_cx(GreenCorner& a, GreenCorner& b) {
    const bool sw = b.x < a.x;
    const GreenCorner lo = green_sel(sw, b, a), hi = green_sel(sw, a, b);
    a = lo;
    b = hi;
}

// The Taylor series of J[x_0 .. x_M] about the mean; u[l] = Re z - x_l, ur their mean, (ur, ui) = ubar, n2 = |ubar|^2.  The mean
// and delta_l = ur - u[l] come from the differences Re z - x_l, which are exact and small close to a corner: ubar then carries a
// relative error of eps, where the rounding of mean(x), eps |x|, would move 1 / ubar by eps |x| / |ubar|^2.
template <int M>
__device__ __forceinline__ Cx green_series(const double (&u)[M + 1], double ur, double ui, double n2) {
    const double s = 1.0 / sqrt(n2);
    double dl[M + 1], H[M + 1];
    double r2 = 0.0;
#pragma unroll
    for (int l = 0; l <= M; ++l) {
        dl[l] = (ur - u[l]) * s;
        H[l] = 1.0;
        r2 = fmax(r2, dl[l] * dl[l]);
    }
    const Cx q = {ur * s, -ui * s};  // 1 / (ubar / |ubar|)
    Cx acc = q, p = q;
    double rk2 = r2;
    for (int k = 1; rk2 >= GREEN_EPS2 && k <= GREEN_KMAX; ++k) {
        H[0] *= dl[0];
#pragma unroll
        for (int l = 1; l <= M; ++l) H[l] = H[l - 1] + dl[l] * H[l];
        p = cx_mul(p, q);
        const double t = GREEN_COEF.c[M - 1][k] * H[M];
        acc.re += t * p.re;
        acc.im += t * p.im;
        rk2 *= r2;
    }
    return {acc.re * s, acc.im * s};
}

// J of two sorted corners
__device__ __forceinline__ Cx green_pair(const GreenCorner& a, const GreenCorner& b, double zr, double zi) {
    const double u[2] = {zr - a.x, zr - b.x};
    const double w = b.x - a.x, ur = 0.5 * (u[0] + u[1]), n2 = ur * ur + zi * zi;
    if (w * w < GREEN_RHO2 * n2) return green_series<1>(u, ur, zi, n2);
    const double iw = 1.0 / w;
    return {(a.lr - b.lr) * iw, (a.li - b.li) * iw};
}

// J of three sorted corners from the J of its two pairs, which only a wide triple reads
__device__ __forceinline__ Cx green_triple(const GreenCorner& a, const GreenCorner& b, const GreenCorner& c, Cx pab, Cx pbc, double zr,
                                           double zi) {
    const double u[3] = {zr - a.x, zr - b.x, zr - c.x};
    const double w = c.x - a.x, ur = (u[0] + u[1] + u[2]) * (1.0 / 3.0), n2 = ur * ur + zi * zi;
    if (w * w < GREEN_RHO2 * n2) return green_series<2>(u, ur, zi, n2);
    const Cx t0 = cx_mul({u[0], zi}, pab), t1 = cx_mul({u[2], zi}, pbc);
    const double f = 2.0 / w;
    return {(t0.re - t1.re) * f, (t0.im - t1.im) * f};
}

// J of a simplex with corners in any order
__device__ __forceinline__ Cx green_simplex(GreenCorner a, GreenCorner b, double zr, double zi) {
    green_cx(a, b);
    return green_pair(a, b, zr, zi);
}
__device__ __forceinline__ Cx green_simplex(GreenCorner a, GreenCorner b, GreenCorner c, double zr, double zi) {
    green_cx(a, b);
    green_cx(b, c);
    green_cx(a, b);
    return green_triple(a, b, c, green_pair(a, b, zr, zi), green_pair(b, c, zr, zi), zr, zi);
}
__device__ __forceinline__ Cx green_simplex(GreenCorner a, GreenCorner b, GreenCorner c, GreenCorner d, double zr, double zi) {
    green_cx(a, b);
    green_cx(c, d);
    green_cx(a, c);
    green_cx(b, d);
    green_cx(b, c);
    const double u[4] = {zr - a.x, zr - b.x, zr - c.x, zr - d.x};
    const double w = d.x - a.x, ur = 0.25 * ((u[0] + u[1]) + (u[2] + u[3])), n2 = ur * ur + zi * zi;
    if (w * w < GREEN_RHO2 * n2) return green_series<3>(u, ur, zi, n2);
    // the two triples share the middle pair
    const Cx p01 = green_pair(a, b, zr, zi), p12 = green_pair(b, c, zr, zi), p23 = green_pair(c, d, zr, zi);
    const Cx j0 = green_triple(a, b, c, p01, p12, zr, zi), j1 = green_triple(b, c, d, p12, p23, zr, zi);
    const Cx t0 = cx_mul({u[0], zi}, j0), t1 = cx_mul({u[3], zi}, j1);
    const double f = 1.5 / w;
    return {(t0.re - t1.re) * f, (t0.im - t1.im) * f};
}

// partial [2 nz][nrows]: column 2 i + {0, 1} the real and imaginary part of the sum at z_i
template <int D>
__global__ __launch_bounds__(256) void ltm_green_kernel(GreenArgs a, double* __restrict__ partial, int64_t nrows) {
    // [zn][2] this block's values of z | [4 waves][zn][2] sums
    extern __shared__ __attribute__((aligned(16))) double ldsg[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NV = 1 << D;  // corners per cell
    const int z0 = (int)blockIdx.z * a.zper;
    const int zn = min(a.zper, a.nz - z0);
    const double* const zl = ldsg;
    double* const acc = ldsg + (size_t)2 * zn * (1 + wave);
    for (int i = threadIdx.x; i < 2 * zn; i += 256) ldsg[i] = a.z[2 * z0 + i];
    for (int i = threadIdx.x; i < 8 * zn; i += 256) ldsg[2 * zn + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const double* __restrict__ const Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    const int64_t tileE = a.E.tile;
    // the whole-grid geometry of ltm_window_kernel: corner `bits` of cell (i1, i2, i3), every index wrapped mod npt
    auto cornerE = [&](int i1, int i2, int i3, int bits) -> double {
        if ((bits & 1) && ++i1 == npt) i1 = 0;
        if (D >= 2 && (bits & 2) && ++i2 == npt) i2 = 0;
        if (D == 3 && (bits & 4) && ++i3 == npt) i3 = 0;
        return Eb[((int64_t)i3 * npt + i2) * tileE + i1];
    };
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        const bool active = k < a.ncell;
        double c[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) c[j] = 0.0;
        if (active) {
            const int64_t line = k <= 0xffffffffll ? (int64_t)((uint32_t)k / (uint32_t)npt) : k / npt;
            const int i1 = (int)(k - line * npt);
            const int i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
            const int i2 = (int)line - i3 * npt;
#pragma unroll
            for (int j = 0; j < NV; ++j) c[j] = cornerE(i1, i2, i3, j);
        }
        for (int iz = 0; iz < zn; ++iz) {
            const double zr = zl[2 * iz], zi = zl[2 * iz + 1];
            double sr = 0.0, si = 0.0;
            if (active) {
                GreenCorner g[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const double ur = zr - c[j];
                    g[j] = {c[j], 0.5 * log(ur * ur + zi * zi), atan2(zi, ur)};
                }
                if constexpr (D == 3) {
                    // the permutation (X, Y, Z) of the axes: corners 0, e_X, e_X + e_Y, (1,1,1); a loop, the corners by selects
#pragma unroll 1
                    for (int t = 0; t < 6; ++t) {
                        const int X = t >> 1, Y = (X + 1 + (t & 1)) % 3;
                        const int bb = (1 << X) | (1 << Y);
                        const GreenCorner ga = green_sel(X == 0, g[1], green_sel(X == 1, g[2], g[4]));
                        const GreenCorner gb = green_sel(bb == 3, g[3], green_sel(bb == 5, g[5], g[6]));
                        const Cx J = green_simplex(g[0], ga, gb, g[7], zr, zi);
                        sr += J.re;
                        si += J.im;
                    }
                } else if constexpr (D == 2) {
#pragma unroll 1
                    for (int t = 0; t < 2; ++t) {
                        const Cx J = green_simplex(g[0], green_sel(t == 0, g[1], g[2]), g[3], zr, zi);
                        sr += J.re;
                        si += J.im;
                    }
                } else {
                    const Cx J = green_simplex(g[0], g[1], zr, zi);
                    sr = J.re;
                    si = J.im;
                }
            }
            // every lane ends with the same bits: a + b == b + a at every level of the butterfly
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                sr += __shfl_xor(sr, off);
                si += __shfl_xor(si, off);
            }
            if (lane == 0) {
                acc[2 * iz] += sr;
                acc[2 * iz + 1] += si;
            }
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = ldsg + 2 * zn;
    const size_t w = (size_t)2 * zn;  // from one wave's sums to the next
    for (int t = threadIdx.x; t < 2 * zn; t += 256)
        partial[(int64_t)(2 * z0 + t) * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
}

using LtmGreenFn = void (*)(GreenArgs, double*, int64_t);
constexpr LtmGreenFn LTM_GREEN[3] = {ltm_green_kernel<1>, ltm_green_kernel<2>, ltm_green_kernel<3>};
}  // namespace

// z_host [nz][2] with Im z != 0, out_host [nz][2].  Im z < 0: the conjugate of the value at conj(z), to the bit.
int launch_ltm_green(abz_ctx* ctx, int n, int d, int npt, PlaneView E, const double* z_host, int nz, double* out_host) {
    GreenArgs a;
    a.E = E;
    a.npt = npt;
    a.ncell = 1;
    for (int j = 0; j < d; ++j) a.ncell *= npt;
    const double weight = 1.0 / ((double)ltm_nsimplex(d) * (double)a.ncell);
    std::vector<double> zup(2 * (size_t)nz);
    for (size_t i = 0; i < (size_t)nz; ++i) {
        zup[2 * i] = z_host[2 * i];
        zup[2 * i + 1] = std::fabs(z_host[2 * i + 1]);
    }
    // the scans' grid: one block row per band, enough blocks to fill the device several times over, few enough partial rows
    const int64_t nblocks = std::min<int64_t>(cdiv64(a.ncell, 256), std::max(64, std::min(2048, 8192 / n)));
    const int64_t nrows = nblocks * n;
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nrows * 2 * (size_t)std::min(nz, LTM_GREEN_CHUNK));
    if (rc) return rc;
    double* partial = ctx->scratch[1].as<double>();
    const double* zdev = nullptr;
    if ((rc = sweep_to_device(ctx, zup.data(), 2 * nz, &zdev))) return rc;
    SumOut so;
    so.host = out_host;
    if (mbox_reserve(ctx) == ABZ_OK && sizeof(double2) * (size_t)nz <= ctx->mbox_cap / 2) {  // the mailbox's result half
        so.map_dev = reinterpret_cast<double2*>(static_cast<char*>(ctx->mbox_dev) + ctx->mbox_cap / 2);
        so.map_host = reinterpret_cast<const double2*>(static_cast<const char*>(ctx->mbox) + ctx->mbox_cap / 2);
    }
    double2* where = nullptr;
    if ((rc = sum_target(ctx, so, 0, nz, &where))) return rc;
    for (int s0 = 0; s0 < nz; s0 += LTM_GREEN_CHUNK) {
        const int cnt = std::min(LTM_GREEN_CHUNK, nz - s0);
        // where the cells give fewer than ~2048 blocks the values of z are dealt to blockIdx.z, at least 4 per block
        const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(2048, nrows), cdiv64(cnt, 4)));
        a.z = zdev + 2 * (size_t)s0;
        a.nz = cnt;
        a.zper = (int)cdiv64(cnt, nsplit);
        const dim3 grid((unsigned)nblocks, (unsigned)n, (unsigned)cdiv64(cnt, a.zper));
        ProfScope ps(ctx, ABZ_K_LTM);
        launch(ctx, LTM_GREEN[d - 1], grid, dim3(256), (unsigned)(sizeof(double) * 10 * (size_t)a.zper), a, partial, nrows);
        ABZ_HIP(hipGetLastError());
        launch(ctx, ltm_final_kernel, dim3((unsigned)(2 * cnt)), dim3(256), 0, (const double*)partial, nrows, weight, 2 * cnt, (int64_t)0,
               reinterpret_cast<double*>(where + s0));
        ABZ_HIP(hipGetLastError());
    }
    if ((rc = sum_deliver(ctx, so, where, 0, nz))) return rc;
    for (size_t i = 0; i < (size_t)nz; ++i)
        if (z_host[2 * i + 1] < 0.0) out_host[2 * i + 1] = -out_host[2 * i + 1];
    return ABZ_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Green's function with matrix elements at complex energies (abz_rule_ltm_green_weighted)
// ---------------------------------------------------------------------------------------------------------------------
// G_A,c(z) = w sum_{cells} sum_{d! simplices} sum_{bands} sum_{i=0..m} A_{c,i} W_i(z), m = d: the element of component c is linear
// inside a simplex like the energy, and W_i is the mean of lambda_i / (z - e) over it.  The uniform density times lambda_i,
// normalised, is Dirichlet(1, .., 2, .., 1), whose image under e is the B-spline with the knot x_i doubled:
//      W_i = J[x_0 .. x_m, x_i](z) / (m + 1)
//  * The J of m + 2 knots with one repeat obeys the recursion above with J[x, x] = 1 / u, and the evaluation rule carries over:
//    a sub-range (a contiguous run of the sorted multiset) narrower than rho |z - mean| is summed by the same Taylor series,
//    now of up to five knots (M = 4): max |delta| <= 4/5 width, the ratio stays below 2/5, (2/5)^k >= 2^-52 up to k = 39, within
//    GREEN_KMAX; the coefficient table has the row m = 4.  Only wider sub-ranges are divided by their width.
//  * Sharing.  The sub-ranges of the m + 1 multisets that hold at most one copy of the doubled knot are the plain ones, P[a][b] =
//    J[x_a .. x_b]: computed once per (simplex, z), d = 3: 3 pairs (from the corner logs), 2 triples, 1 quadruple.  Those that
//    hold both copies, D_i[a][b] = J[x_a .. x_i, x_i .. x_b] with a <= i <= b, start from D_i[i][i] = 1 / u_i and grow by
//      D_i[a][b] = M / (M-1) (u_a lo - u_b hi) / (x_b - x_a),   M = b - a + 1,
//      lo = b > i ? D_i[a][b-1] : P[a][b],   hi = a < i ? D_i[a+1][b] : P[a][b]
//    (dropping the last or the first knot): 16 of them in 3-D, 6 in 2-D, 2 in 1-D.  Every sub-range is evaluated whether or not a
//    wider one turns out narrow and ignores it: each is accurate by itself.  One shortcut comes first: where all m + 1 whole
//    multisets are narrow the weights are m + 1 series and nothing else is formed (150^3 SVO grid, 256 z, one component:
//    2790 ms without it, 1222 ms with it).
//  * Shape (ltm_green_w_kernel<D, NC>).  The cell walk, the corner geometry, the z list in LDS, blockIdx.z and the reduction are
//    ltm_green_kernel's; the 2^d corner energies and the NC 2^d corner elements of a group of NC components stay in registers
//    (LtmElems::load through PlaneView / acomp), the sort of a simplex carries each corner's log and its NC elements, the m + 1
//    weights of a (simplex, z) are formed once and every component contracts with them.  Groups as in ltm_scan: 4s, a 2, a 1.
//    LDS: [zn][2] z | [4 waves][zn][NC][2] sums, so a launch takes green_w_chunk(NC) = 512 / 291 / 154 values of z.
//    1 / (m + 1) goes into the scale of ltm_final_kernel.
namespace {
constexpr int green_w_chunk(int nc) {
    const size_t fit = LTM_LDS_MAX / (sizeof(double) * (size_t)(2 + 8 * nc));
    return fit < (size_t)LTM_GREEN_CHUNK ? (int)fit : LTM_GREEN_CHUNK;
}
static_assert(sizeof(double) * (2 + 8 * 1) * green_w_chunk(1) <= LTM_LDS_MAX && sizeof(double) * (2 + 8 * 2) * green_w_chunk(2) <= LTM_LDS_MAX &&
                  sizeof(double) * (2 + 8 * 4) * green_w_chunk(4) <= LTM_LDS_MAX,
              "the z list and the four waves' sums of every component group fit the scans' LDS");
static_assert(green_w_chunk(4) >= 4 && green_w_chunk(4) <= green_w_chunk(2) && green_w_chunk(2) <= green_w_chunk(1), "chunks shrink with NC");

struct GreenWArgs {
    GreenArgs g;
    PlaneView A;
    int64_t acomp;  // doubles from a band's plane of one component to its plane of the next: n * A.pitch
    int aplane0;    // first element plane of this launch: (its first component) * n
};

// what the sort of a simplex carries per corner: the energy, log(z - energy) and the NC elements
template <int NC>
struct GreenWCorner {
    GreenCorner g;
    LtmVec<NC> a;
};
template <int NC>
__device__ __forceinline__ GreenWCorner<NC> green_wsel(bool first, const GreenWCorner<NC>& p, const GreenWCorner<NC>& q) {
    GreenWCorner<NC> r;
    r.g = green_sel(first, p.g, q.g);
#pragma unroll
    for (int c = 0; c < NC; ++c) r.a.v[c] = first ? p.a.v[c] : q.a.v[c];
    return r;
}
template <int NC>
__device__ __forceinline__ void green_wcx(GreenWCorner<NC>& p, GreenWCorner<NC>& q) {
    const bool sw = q.g.x < p.g.x;
    const GreenWCorner<NC> lo = green_wsel(sw, q, p), hi = green_wsel(sw, p, q);
    p = lo;
    q = hi;
}

// f(integral_constant<int, 0>) ... f(integral_constant<int, N - 1>): loops whose index is a template argument
template <int N, class F>
__device__ __forceinline__ void green_for(F&& f) {
    if constexpr (N > 0) {
        green_for<N - 1>(f);
        f(std::integral_constant<int, N - 1>{});
    }
}

// J of the M + 1 >= 3 sorted knots with u[l] = Re z - knot l and width w, from `lo` (the J without the last knot) and `hi`
// (without the first), which only a wide range reads
template <int M>
__device__ __forceinline__ double green_mean(const double (&u)[M + 1]) {
    double ur = u[0];
#pragma unroll
    for (int l = 1; l <= M; ++l) ur += u[l];
    return ur * (1.0 / (double)(M + 1));
}
template <int M>
__device__ __forceinline__ Cx green_node(const double (&u)[M + 1], double w, Cx lo, Cx hi, double zi) {
    const double ur = green_mean<M>(u), n2 = ur * ur + zi * zi;
    if (w * w < GREEN_RHO2 * n2) return green_series<M>(u, ur, zi, n2);
    const Cx t0 = cx_mul({u[0], zi}, lo), t1 = cx_mul({u[M], zi}, hi);
    const double f = ((double)M / (double)(M - 1)) / w;
    return {(t0.re - t1.re) * f, (t0.im - t1.im) * f};
}

// (m + 1) W_i = J[x_0 .. x_m, x_i] of the NK = m + 1 sorted corners g
template <int NK>
__device__ __forceinline__ void green_weights(const GreenCorner (&g)[NK], double zr, double zi, Cx (&W)[NK]) {
    double u[NK];
#pragma unroll
    for (int l = 0; l < NK; ++l) u[l] = zr - g[l].x;
    // The m + 1 whole multisets first.  Where all of them are narrow -- a fine grid away from the corners' energies: most simplices
    // -- each is its series and no sub-range is read; the value is the one the general path below gives (green_node makes the
    // same decision from the same numbers).
    {
        const double w = g[NK - 1].x - g[0].x;
        double uu[NK][NK + 1], ur[NK], n2[NK];
        bool narrow = true;
#pragma unroll
        for (int i = 0; i < NK; ++i) {
#pragma unroll
            for (int l = 0; l <= NK; ++l) uu[i][l] = u[l - (l > i ? 1 : 0)];
            ur[i] = green_mean<NK>(uu[i]);
            n2[i] = ur[i] * ur[i] + zi * zi;
            narrow = narrow && w * w < GREEN_RHO2 * n2[i];
        }
        if (narrow) {
#pragma unroll
            for (int i = 0; i < NK; ++i) W[i] = green_series<NK>(uu[i], ur[i], zi, n2[i]);
            return;
        }
    }
    Cx P[NK][NK];  // a <= b: J[x_a .. x_b]; P[a][a] = 1 / u_a
#pragma unroll
    for (int l = 0; l < NK; ++l) {
        const double s = 1.0 / (u[l] * u[l] + zi * zi);
        P[l][l] = {u[l] * s, -zi * s};
    }
    green_for<NK - 1>([&](auto L_) {
        constexpr int L = decltype(L_)::value + 1;
        green_for<NK - L>([&](auto a_) {
            constexpr int a = decltype(a_)::value, b = a + L;
            if constexpr (L == 1) {
                P[a][b] = green_pair(g[a], g[b], zr, zi);
            } else {
                double uu[L + 1];
#pragma unroll
                for (int l = 0; l <= L; ++l) uu[l] = u[a + l];
                P[a][b] = green_node<L>(uu, g[b].x - g[a].x, P[a][b - 1], P[a + 1][b], zi);
            }
        });
    });
    green_for<NK>([&](auto i_) {
        constexpr int i = decltype(i_)::value;
        Cx Dd[NK][NK];  // a <= i <= b: J[x_a .. x_i, x_i .. x_b]
        Dd[i][i] = P[i][i];
        green_for<NK - 1>([&](auto L_) {
            constexpr int L = decltype(L_)::value + 1;
            green_for<NK - L>([&](auto a_) {
                constexpr int a = decltype(a_)::value, b = a + L;
                if constexpr (a <= i && i <= b) {
                    constexpr int M = L + 1;
                    double uu[M + 1];
#pragma unroll
                    for (int l = 0; l <= M; ++l) uu[l] = u[a + l - (a + l > i ? 1 : 0)];
                    const Cx lo = b > i ? Dd[a][b - 1] : P[a][b];
                    const Cx hi = a < i ? Dd[a + 1][b] : P[a][b];
                    Dd[a][b] = green_node<M>(uu, g[b].x - g[a].x, lo, hi, zi);
                }
            });
        });
        W[i] = Dd[0][NK - 1];
    });
}

// sum_i A_{c,i} (m + 1) W_i of a simplex with corners in any order, added to (sr, si)[c]
template <int NK, int NC>
__device__ __forceinline__ void green_wsimplex(GreenWCorner<NC> (&q)[NK], double zr, double zi, double (&sr)[NC], double (&si)[NC]) {
    if constexpr (NK == 2) {
        green_wcx(q[0], q[1]);
    } else if constexpr (NK == 3) {
        green_wcx(q[0], q[1]);
        green_wcx(q[1], q[2]);
        green_wcx(q[0], q[1]);
    } else {
        green_wcx(q[0], q[1]);
        green_wcx(q[2], q[3]);
        green_wcx(q[0], q[2]);
        green_wcx(q[1], q[3]);
        green_wcx(q[1], q[2]);
    }
    GreenCorner g[NK];
#pragma unroll
    for (int l = 0; l < NK; ++l) g[l] = q[l].g;
    Cx W[NK];
    green_weights<NK>(g, zr, zi, W);
#pragma unroll
    for (int c = 0; c < NC; ++c) {
#pragma unroll
        for (int l = 0; l < NK; ++l) {
            sr[c] += q[l].a.v[c] * W[l].re;
            si[c] += q[l].a.v[c] * W[l].im;
        }
    }
}

// partial [2 NC nz][nrows]: column (i NC + c) 2 + {0, 1} the real and imaginary part of component c's sum at z_i
template <int D, int NC>
__global__ __launch_bounds__(256) void ltm_green_w_kernel(GreenWArgs wa, double* __restrict__ partial, int64_t nrows) {
    // [zn][2] this block's values of z | [4 waves][zn][NC][2] sums
    extern __shared__ __attribute__((aligned(16))) double ldsw[];
    const GreenArgs& a = wa.g;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NV = 1 << D;  // corners per cell
    using Load = LtmElems<NC, false>;
    using Corner = GreenWCorner<NC>;
    const int z0 = (int)blockIdx.z * a.zper;
    const int zn = min(a.zper, a.nz - z0);
    const double* const zl = ldsw;
    double* const acc = ldsw + (size_t)2 * zn * (1 + NC * wave);
    for (int i = threadIdx.x; i < 2 * zn; i += 256) ldsw[i] = a.z[2 * z0 + i];
    for (int i = threadIdx.x; i < 8 * NC * zn; i += 256) ldsw[2 * zn + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const double* __restrict__ const Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    const double* __restrict__ const Ab = wa.A.base + (int64_t)(wa.aplane0 + (int)blockIdx.y) * wa.A.pitch;
    const int64_t tileE = a.E.tile, tileA = wa.A.tile, acomp = wa.acomp;
    // the whole-grid geometry of ltm_window_kernel: corner `bits` of cell (i1, i2, i3), every index wrapped mod npt
    auto wrap = [&](int& i1, int& i2, int& i3, int bits) {
        if ((bits & 1) && ++i1 == npt) i1 = 0;
        if (D >= 2 && (bits & 2) && ++i2 == npt) i2 = 0;
        if (D == 3 && (bits & 4) && ++i3 == npt) i3 = 0;
    };
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        const bool active = k < a.ncell;
        double c[NV];
        LtmVec<NC> ca[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            c[j] = 0.0;
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) ca[j].v[cc] = 0.0;
        }
        if (active) {
            const int64_t line = k <= 0xffffffffll ? (int64_t)((uint32_t)k / (uint32_t)npt) : k / npt;
            const int i1 = (int)(k - line * npt);
            const int i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
            const int i2 = (int)line - i3 * npt;
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                int j1 = i1, j2 = i2, j3 = i3;
                wrap(j1, j2, j3, j);
                c[j] = Eb[((int64_t)j3 * npt + j2) * tileE + j1];
                ca[j] = Load::load(Ab + ((int64_t)j3 * npt + j2) * tileA + j1, acomp);
            }
        }
        for (int iz = 0; iz < zn; ++iz) {
            const double zr = zl[2 * iz], zi = zl[2 * iz + 1];
            double sr[NC], si[NC];
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) sr[cc] = si[cc] = 0.0;
            if (active) {
                Corner g[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const double ur = zr - c[j];
                    g[j].g = {c[j], 0.5 * log(ur * ur + zi * zi), atan2(zi, ur)};
                    g[j].a = ca[j];
                }
                if constexpr (D == 3) {
                    // the permutation (X, Y, Z) of the axes: corners 0, e_X, e_X + e_Y, (1,1,1); a loop, the corners by selects
#pragma unroll 1
                    for (int t = 0; t < 6; ++t) {
                        const int X = t >> 1, Y = (X + 1 + (t & 1)) % 3;
                        const int bb = (1 << X) | (1 << Y);
                        Corner q[4] = {g[0], green_wsel(X == 0, g[1], green_wsel(X == 1, g[2], g[4])),
                                       green_wsel(bb == 3, g[3], green_wsel(bb == 5, g[5], g[6])), g[7]};
                        green_wsimplex<4, NC>(q, zr, zi, sr, si);
                    }
                } else if constexpr (D == 2) {
#pragma unroll 1
                    for (int t = 0; t < 2; ++t) {
                        Corner q[3] = {g[0], green_wsel(t == 0, g[1], g[2]), g[3]};
                        green_wsimplex<3, NC>(q, zr, zi, sr, si);
                    }
                } else {
                    Corner q[2] = {g[0], g[1]};
                    green_wsimplex<2, NC>(q, zr, zi, sr, si);
                }
            }
            // every lane ends with the same bits: a + b == b + a at every level of the butterfly
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) {
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) {
                    sr[cc] += __shfl_xor(sr[cc], off);
                    si[cc] += __shfl_xor(si[cc], off);
                }
                if (lane == 0) {
                    acc[2 * (iz * NC + cc)] += sr[cc];
                    acc[2 * (iz * NC + cc) + 1] += si[cc];
                }
            }
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = ldsw + 2 * zn;
    const size_t w = (size_t)2 * NC * zn;  // from one wave's sums to the next
    for (int t = threadIdx.x; t < 2 * NC * zn; t += 256)
        partial[((int64_t)2 * NC * z0 + t) * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
}

using LtmGreenWFn = void (*)(GreenWArgs, double*, int64_t);
// [d - 1][NC = 1, 2, 4]
constexpr LtmGreenWFn LTM_GREEN_W[3][3] = {
    {ltm_green_w_kernel<1, 1>, ltm_green_w_kernel<1, 2>, ltm_green_w_kernel<1, 4>},
    {ltm_green_w_kernel<2, 1>, ltm_green_w_kernel<2, 2>, ltm_green_w_kernel<2, 4>},
    {ltm_green_w_kernel<3, 1>, ltm_green_w_kernel<3, 2>, ltm_green_w_kernel<3, 4>},
};
}  // namespace

// z_host [nz][2] with Im z != 0, A the element planes of `ncomp` components (A = E, ncomp = 1: the energy), out_host
// [nz][ncomp][2].  Im z < 0: the conjugate of the value at conj(z), to the bit (the elements are real).
int launch_ltm_green_weighted(abz_ctx* ctx, int n, int d, int npt, PlaneView E, PlaneView A, int ncomp, const double* z_host, int nz,
                              double* out_host) {
    GreenWArgs a;
    a.g.E = E;
    a.g.npt = npt;
    a.g.ncell = 1;
    for (int j = 0; j < d; ++j) a.g.ncell *= npt;
    a.A = A;
    a.acomp = (int64_t)n * A.pitch;
    // of a simplex and, of its d + 1 corner weights, the 1 / (m + 1)
    const double weight = 1.0 / ((double)ltm_nsimplex(d) * (double)a.g.ncell * (double)(d + 1));
    std::vector<double> zup(2 * (size_t)nz);
    for (size_t i = 0; i < (size_t)nz; ++i) {
        zup[2 * i] = z_host[2 * i];
        zup[2 * i + 1] = std::fabs(z_host[2 * i + 1]);
    }
    // the scans' grid: one block row per band, enough blocks to fill the device several times over, few enough partial rows
    const int64_t nblocks = std::min<int64_t>(cdiv64(a.g.ncell, 256), std::max(64, std::min(2048, 8192 / n)));
    const int64_t nrows = nblocks * n;
    size_t pmax = 0;
    for (int nc : {1, 2, 4})
        if (nc <= ncomp) pmax = std::max(pmax, (size_t)std::min(nz, green_w_chunk(nc)) * (size_t)(2 * nc));
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nrows * pmax);
    if (rc) return rc;
    double* partial = ctx->scratch[1].as<double>();
    const double* zdev = nullptr;
    if ((rc = sweep_to_device(ctx, zup.data(), 2 * nz, &zdev))) return rc;
    const size_t ncols = (size_t)nz * (size_t)ncomp;
    SumOut so;
    so.host = out_host;
    if (mbox_reserve(ctx) == ABZ_OK && sizeof(double2) * ncols <= ctx->mbox_cap / 2) {  // the mailbox's result half
        so.map_dev = reinterpret_cast<double2*>(static_cast<char*>(ctx->mbox_dev) + ctx->mbox_cap / 2);
        so.map_host = reinterpret_cast<const double2*>(static_cast<const char*>(ctx->mbox) + ctx->mbox_cap / 2);
    }
    double2* where = nullptr;
    if ((rc = sum_target(ctx, so, 0, (int64_t)ncols, &where))) return rc;
    // groups of 4 components, then 2, then 1; every group walks the grid once per chunk of z
    for (int c0 = 0; c0 < ncomp;) {
        const int nc = ncomp - c0 >= 4 ? 4 : (ncomp - c0 >= 2 ? 2 : 1);
        const int CH = green_w_chunk(nc);
        a.aplane0 = c0 * n;
        for (int s0 = 0; s0 < nz; s0 += CH) {
            const int cnt = std::min(CH, nz - s0);
            // where the cells give fewer than ~2048 blocks the values of z are dealt to blockIdx.z, at least 4 per block
            const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(2048, nrows), cdiv64(cnt, 4)));
            a.g.z = zdev + 2 * (size_t)s0;
            a.g.nz = cnt;
            a.g.zper = (int)cdiv64(cnt, nsplit);
            const dim3 grid((unsigned)nblocks, (unsigned)n, (unsigned)cdiv64(cnt, a.g.zper));
            ProfScope ps(ctx, ABZ_K_LTM);
            launch(ctx, LTM_GREEN_W[d - 1][nc >> 1], grid, dim3(256), (unsigned)(sizeof(double) * (size_t)(2 + 8 * nc) * (size_t)a.g.zper), a,
                   partial, nrows);
            ABZ_HIP(hipGetLastError());
            // column (i nc + c) 2 + t of the launch -> out[s0 + i][c0 + c][t]
            launch(ctx, ltm_final_kernel, dim3((unsigned)(2 * nc * cnt)), dim3(256), 0, (const double*)partial, nrows, weight, 2 * nc,
                   (int64_t)2 * ncomp, reinterpret_cast<double*>(where + ((size_t)s0 * (size_t)ncomp + (size_t)c0)));
            ABZ_HIP(hipGetLastError());
        }
        c0 += nc;
    }
    if ((rc = sum_deliver(ctx, so, where, 0, (int64_t)ncols))) return rc;
    for (size_t i = 0; i < (size_t)nz; ++i)
        if (z_host[2 * i + 1] < 0.0)
            for (size_t c = 0; c < (size_t)ncomp; ++c) out_host[2 * (i * (size_t)ncomp + c) + 1] = -out_host[2 * (i * (size_t)ncomp + c) + 1];
    return ABZ_OK;
}

int launch_ltm(abz_ctx* ctx, int n, int d, int npt, PlaneView E, const double* Es_host, int nE, bool states, double* out_host,
               const LtmSlab* slab) {
    return ltm_scan(ctx, "launch_ltm", n, d, npt, E, nullptr, 1, Es_host, nE, states ? ABZ_LTM_STATES : ABZ_LTM_DOS, out_host, slab);
}

int launch_ltm_weighted(abz_ctx* ctx, int n, int d, int npt, PlaneView E, PlaneView A, int ncomp, const double* Es_host, int nE,
                        int what, double* out_host, const LtmSlab* slab) {
    return ltm_scan(ctx, "launch_ltm_weighted", n, d, npt, E, &A, ncomp, Es_host, nE, what, out_host, slab);
}

int launch_ltm_repack(abz_ctx* ctx, const double* src_dev, PlaneView A, int plane0, int n, int64_t nk) {
    ProfScope ps(ctx, ABZ_K_LTM);
    launch(ctx, ltm_repack_kernel, dim3((unsigned)cdiv64(nk * n, 256)), dim3(256), 0, src_dev, A, plane0, n, nk);
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

int launch_ltm_minmax(abz_ctx* ctx, int n, PlaneView E, int64_t nk, double* emin, double* emax) {
    const int nb = (int)std::min<int64_t>(256, cdiv64(nk * n, 256));
    int rc = ctx->scratch[1].reserve(sizeof(double) * 2 * (size_t)nb);
    if (rc) return rc;
    double* part = ctx->scratch[1].as<double>();
    {
        ProfScope ps(ctx, ABZ_K_LTM);
        launch(ctx, ltm_minmax_kernel, dim3((unsigned)nb), dim3(256), 0, E, n, nk, part);
        ABZ_HIP(hipGetLastError());
    }
    std::vector<double> h(2 * (size_t)nb);
    ABZ_HIP(hipMemcpyAsync(h.data(), part, sizeof(double) * h.size(), hipMemcpyDeviceToHost, ctx->stream));
    ABZ_HIP(hipStreamSynchronize(ctx->stream));
    double mn = h[0], mx = h[1];
    for (int b = 1; b < nb; ++b) {
        mn = std::min(mn, h[2 * (size_t)b]);
        mx = std::max(mx, h[2 * (size_t)b + 1]);
    }
    *emin = mn;
    *emax = mx;
    return ABZ_OK;
}

int launch_ltm_orbit_map(abz_ctx* ctx, int npt, int d, const int32_t* syms, int nsyms, const int32_t* idx, int64_t nk, int32_t* rank,
                         int32_t* node_of, int* missing_dev) {
    if (nsyms > 48 || d > 3 || d < 1) {
        set_error("abz_rule_ltm_unfold: at most 48 symmetries of a <= 3-d lattice");
        return ABZ_ERR_UNSUPPORTED;
    }
    SymArgs a;
    sym_args_init(a, npt, d, syms, nsyms);
    ABZ_HIP(hipMemsetAsync(rank, 0xff, sizeof(int32_t) * (size_t)a.N, ctx->stream));  // -1: not a node
    ABZ_HIP(hipMemsetAsync(missing_dev, 0, sizeof(int), ctx->stream));
    ProfScope ps(ctx, ABZ_K_LTM);
    launch(ctx, ltm_rank_kernel, dim3((unsigned)cdiv64(nk, 256)), dim3(256), 0, idx, nk, d, npt, a.N, rank);
    ABZ_HIP(hipGetLastError());
    launch(ctx, ltm_orbit_kernel, dim3((unsigned)cdiv64(a.N, 256)), dim3(256), 0, a, (const int32_t*)rank, node_of, missing_dev);
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

int launch_ltm_unfold(abz_ctx* ctx, PlaneView src, PlaneView dst, const int32_t* node_of, int n, int npt, int64_t nlines) {
    const int chunks = (dst.row + 63) / 64;
    const int64_t nunits = nlines * chunks;
    ProfScope ps(ctx, ABZ_K_LTM);
    launch(ctx, ltm_unfold_kernel, dim3((unsigned)cdiv64(nunits, 4)), dim3(256), 0, src, dst, node_of, n, npt, chunks, nunits);
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

int ltm_fermi(abz_ctx* ctx, int n, int d, int npt, PlaneView E, int64_t nk, double nstates, double tol, double* E_F, double* N_F) {
    double lo = 0.0, hi = 0.0;
    int rc = launch_ltm_minmax(ctx, n, E, nk, &lo, &hi);
    if (rc) return rc;
    const double hi_all = hi;
    const double target = nstates * (1.0 - 1e-12);
    constexpr int M = 512;
    std::vector<double> Es(M), N(M);
    double Nhi = (double)n;
    // every scan keeps the sub-interval (E_{i-1}, E_i] of its M samples with N(E_{i-1}) < target <= N(E_i): 511 times
    // narrower per launch
    for (int it = 0; it < 64; ++it) {
        const double width = hi - lo;
        int m = M;
        if (!(width > 0.0)) m = 1;
        for (int i = 0; i < m; ++i) Es[(size_t)i] = i == m - 1 ? hi : lo + width * ((double)i / (double)(M - 1));
        if ((rc = launch_ltm(ctx, n, d, npt, E, Es.data(), m, true, N.data()))) return rc;
        int i = 0;
        while (i < m - 1 && !(N[(size_t)i] >= target)) ++i;  // the upper end stands for "none": N(hi) >= target was seen before
        Nhi = N[(size_t)i];
        const double nlo = i > 0 ? Es[(size_t)i - 1] : lo, nhi = Es[(size_t)i];
        if (i == 0) {  // already the lower end holds the states (first scan: a flat band at the bottom)
            hi = nhi;
            break;
        }
        const bool shrunk = nhi - nlo < width;
        lo = nlo;
        hi = nhi;
        if (hi - lo <= tol || !shrunk) break;
    }
    // Below a gap the search stops short of the band top: under a 3-D maximum N(top - x) = 1 - c x^3 reaches the target a
    // distance (1e-12 / c)^(1/3), about 1e-4, below it, and in f64 N cannot tell x < 1e-5 from 0.  The DOS can: g(E) is
    // exactly 0 where no simplex straddles E (nothing is added to its sum) and positive below the top.  So if g vanishes
    // at a sample above `hi` while N there is still nstates to the same slack -- a gap, not the next band edge of a
    // metal -- the same 511-fold narrowing on "g == 0" finds the lowest such energy, the band top, to within tol.
    const double emax = hi_all, upper = nstates * (1.0 + 1e-12);
    if (emax > hi) {
        std::vector<double>& G = N;
        double a = hi, b = emax;
        bool gap = false;
        for (int it = 0; it < 64; ++it) {
            const double width = b - a;
            for (int i = 0; i < M; ++i) Es[(size_t)i] = i == M - 1 ? b : a + width * ((double)i / (double)(M - 1));
            if ((rc = launch_ltm(ctx, n, d, npt, E, Es.data(), M, false, G.data()))) return rc;
            int i = 0;
            while (i < M - 1 && G[(size_t)i] != 0.0) ++i;
            if (it == 0) {
                if (G[(size_t)i] != 0.0 || i == 0) break;  // no zero of g above hi, or hi itself already has one
                double Nz = 0.0;
                if ((rc = launch_ltm(ctx, n, d, npt, E, &Es[(size_t)i], 1, true, &Nz))) return rc;
                if (Nz > upper) break;  // states in between: the zero belongs to a higher gap
                gap = true;
            }
            if (i == 0) {  // (rounding: the lower end had g > 0 in the scan before)
                b = a;
                break;
            }
            const double na = Es[(size_t)i - 1], nb = Es[(size_t)i];
            const bool shrunk = nb - na < width;
            a = na;
            b = nb;
            if (b - a <= tol || !shrunk) break;
        }
        if (gap) {
            hi = b;
            if ((rc = launch_ltm(ctx, n, d, npt, E, &hi, 1, true, &Nhi))) return rc;
        }
    }
    *E_F = hi;
    if (N_F) *N_F = Nhi;
    return ABZ_OK;
}

}  // namespace abz
