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
//    LtmElems<NC, CORR> (NC matrix elements, next item).  The policy says what a corner carries (elements: ltm_load of ltm_device.h), picks the simplex routine and
//    says what a cell without an energy in its window adds to the step histogram; the cell walk, the corner geometry (whole
//    grid or slab with its halo plane), the window, the queue and the write-out are the kernel's and exist once.  One final
//    and one prefix kernel serve both (the plain scan is one component), one host function (ltm_scan) launches them, and the
//    table LTM_WINDOWS lists the compiled instantiations: a scan that is not in it is refused.
//    The routines every tetrahedron scan shares -- ltm_first, ltm_add and the simplex routines of the element payload -- live in
//    ltm_simplex_device.h, which the occupied pair scan (kernels_ltm_pairs_occ.hip) reads too.
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
#include "ltm_device.h"
#include "ltm_simplex_device.h"
#include "rows_device.h"
#include "sym_image.h"

namespace abz {

namespace {

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

// ---------------------------------------------------------------------------------------------------------------------
// The scan: one kernel, two payloads
// ---------------------------------------------------------------------------------------------------------------------
// A payload says what a corner carries besides its energy (Vec), which routine takes a simplex (the overload of
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
    // The geometry, for energies and elements alike: corner `bits` of cell (i1, i2, i3), which become the corner's own indices.
    // Whole grid: ltm_wrap.  SLAB: the outermost index is local to the slab's nz planes and does not wrap; true: the corner lies
    // behind plane nz - 1, in the halo plane, at column i1 of its line i2 (d = 2: of its only line, 0).
    auto corner = [&](int& i1, int& i2, int& i3, int bits) -> bool {
        if constexpr (SLAB) {
            if ((bits & 1) && ++i1 == npt) i1 = 0;
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
            ltm_wrap<D>(i1, i2, i3, bits, npt);
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
            return ltm_load<P::NC>(SLAB && halo ? AHb + (int64_t)i2 * htileA + i1 : Ab + ((int64_t)i3 * npt + i2) * tileA + i1, acomp);
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
            const LtmCell cell = ltm_cell<D>(k, npt);
            i1 = cell.i1;
            i2 = cell.i2;
            i3 = cell.i3;
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
            const LtmCell cq = ltm_cell<D>(base + (q & 255u), npt);
            const int q1 = cq.i1, q2 = cq.i2, q3 = cq.i3;
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
// (ggr_final_kernel's); launch_ltm_final below launches it for every tetrahedron file
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
}  // namespace

int launch_ltm_final(abz_ctx* ctx, const double* partial, int64_t nrows, double scale, int ncols, int cnt, int64_t ostride, double* out) {
    launch(ctx, ltm_final_kernel, dim3((unsigned)ncols), dim3(256), 0, partial, nrows, scale, cnt, ostride, out);
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

int launch_ltm_prefix(abz_ctx* ctx, const double* col, int nE, int nc, double weight, int64_t ostride, double* out) {
    launch(ctx, ltm_prefix_kernel, dim3((unsigned)nc), dim3(256), 0, col, nE, nc, weight, ostride, out);
    ABZ_HIP(hipGetLastError());
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
