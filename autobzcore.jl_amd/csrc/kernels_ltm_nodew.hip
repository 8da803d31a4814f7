// Linear tetrahedron method (gfx950 only): Bloechl's integration weights w_b(k; E) per grid point and band, in gather form.
//
// The scans of kernels_ltm.hip walk the d! npt^d simplices, form the corner weights of each and contract them at once with what is
// attached.  Here the weights themselves are the result: the numbers with
//      N_A(E) = sum_k sum_b w_b(k; E) A_b(k)          (and g_A, and N_A with the curvature correction)
// for ANY A, as a resident block tiled like an element block of abz_rule_ltm_elements: plane iE n + b of a grid line's tile is
// the weight of band b at energy iE, pitch E.row, padding columns zero.  Mesh, band convention, half-open regions and the simplex
// weight 1 / (d! npt^d) are those of kernels_ltm.hip; the formulas are restated here on purpose, as LtmPlain and LtmElems restate
// each other: nothing of that file is touched, and its compiled scans stay what they were.
//
//  * Gather.  The weight of node k is the sum over the (d+1)! Kuhn simplices that contain k of what the simplex gives that corner:
//    for every permutation (X, Y, Z) of the axes and every position j = 0..d of k in the chain
//      j = 0: k, k + X, k + X + Y, k + X + Y + Z        j = 1: k - X, k, k + Y, k + Y + Z
//      j = 2: k - X - Y, k - Y, k, k + Z                j = 3: k - X - Y - Z, k - Y - Z, k - Z, k
//    (d = 2, d = 1: the same with one and two axes fewer), 24, 6 or 2 simplices whose corners are among the 3^d neighbours k + delta,
//    every index wrapped mod npt.  At npt = 2 the neighbours k + 1 and k - 1 are the same node and both simplices exist, as in the
//    scans.  One thread per (grid point, band), the band in blockIdx.y; the wraps of the axes are independent, so a neighbour's
//    address is the node's own plus one precomputed offset per axis, and the permutation loop selects those offsets: the 3 d!
//    neighbour values of a permutation are loaded as they are needed (they are the neighbours' own values: L1 / L2 hits), nothing
//    is indexed at run time and nothing goes to scratch (DESIGN section 4e has the compiler's resource report).
//  * Which sorted corner is k: the compare-exchange network that sorts the corner energies swaps a one-hot flag along.
//  * Corner weights (those of LtmElems<NC, false>), sorted e1 <= .. <= e_{d+1}, t_ij = (E - e_i) / (e_j - e_i),
//    s_j = (e_last - E) / (e_last - e_j), unit = one simplex:
//      d = 3, e1 <= E < e2: q = t12 t13 t14 / 4, N: w_j = q t_1j, w_1 = 4 q - sum;  g: q = t13 t14 / e21, w_j = q t_1j, w_1 = 3 q - sum
//             e2 <= E < e3: the part below E is a prism cut into the tetrahedra (1, P13, P14, 2) (P13, P14, 2, P23) (P14, 2, P23, P24)
//             of volumes v1 = t13 t14, v2 = t14 t23 (1 - t13), v3 = (1 - t14) t23 t24, a quarter of each to its vertices; the cut is
//             the triangles (P13, P14, P23) (P14, P23, P24) with densities 3 t13 (1 - t23) / e41, 3 t23 (1 - t24) / e41, a third of
//             each to its vertices; a vertex P_ij hands (1 - t_ij, t_ij) of its share to the corners i, j
//             e3 <= E < e4: the mirror image of the first region from corner 4, N: w = 1/4 - (that)
//      d = 2, d = 1: the same with one and two corners fewer.
//    ABZ_LTM_STATES: a simplex wholly below E (e_max <= E, a flat one included) gives 1 / (d+1) to each corner.  These are counted
//    as integers and divided once: a node whose whole neighbourhood lies below E weighs (d+1)! / (d+1) / (d! npt^d) = 1 / npt^d to
//    two roundings, one whose neighbourhood lies above E exactly 0.0.  ABZ_LTM_DOS: a flat simplex gives nothing.
//    ABZ_LTM_STATES_CORRECTED: plus g_T(E) f_d (sum_l e_l - (d+1) e_own) inside the simplex's window e_1 <= E < e_{d+1},
//    f_d = 1 / (2 (d+1)(d+2)): kappa_T of the scans split by corner; g_T from the reciprocals at hand.
//  * Energies.  A launch takes a compile-time group of NE = 1 or 4 energies (by value, no list in memory): the sort and the
//    reciprocals of a simplex serve the group, the NE accumulators and counters stay in registers.  A node whose 3^d neighbourhood
//    holds none of the group's energies between its smallest and largest eigenvalue is finished after those 3^d loads (measured,
//    most of the grid at one energy), and a simplex that holds none inside its window forms no reciprocal.
//  * No atomics anywhere: a thread sums its simplices in program order and two calls write the same bits.
//  * ltm_nodew_dot_kernel: sum_k sum_b w_b(k; E_i) A_{c,b}(k) against the attached element block, [nE][ncomp]; one pass over the
//    weights (blockIdx.y = energy, every component of a node contracted from one load of the weight), fixed-order two-stage
//    reduction (a butterfly over the wave, the four waves in order, then one block per column: launch_ltm_final), results
//    through the pinned mailbox with one synchronisation.
//  * ltm_nodew_fold_kernel: for a rule of abz_rule_ltm_unfold, the weights summed over each orbit onto the source rule's nodes.
//    The Kuhn mesh is invariant under 12 of the 48 cubic operations only, so w(S k) != w(k) in general and the fold is a plain sum
//    over the orbit, not multiplicity x w.  The inverse of the rule's orbit map (for every node the grid points of its orbit,
//    ascending) is built once on the host by a counting sort and kept on the device; one thread per (node, band, energy) walks
//    its list in that order: no atomics, the same bits at every call.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "abz_internal.h"
#include "ltm_device.h"

namespace abz {

namespace {

struct NodeWArgs {
    PlaneView E, W;   // eigenvalue planes; the weight block (nE n planes per tile, pitch = row)
    int64_t nlines;   // npt^(d-1)
    int npt;
    int plane0;       // first weight plane of this launch: (its first energy) * n
    int n;
    double weight;    // 1 / (d! npt^d)
    double Es[4];     // the launch's energies (NE of them)
};

// compare-exchange of two corners: the energies, and the flag "this corner is the node itself" with them
__device__ __forceinline__ void nodew_cx(double& ea, double& eb, bool& oa, bool& ob) {
    const bool sw = eb < ea;
    const double lo = sw ? eb : ea, hi = sw ? ea : eb;
    const bool x = sw ? ob : oa, y = sw ? oa : ob;
    ea = lo;
    eb = hi;
    oa = x;
    ob = y;
}

// One tetrahedron: the node's own energy e0 and its three other corners in any order.  acc[i] += the weight the simplex gives the
// node at energy En[i] (unit = one simplex), full[i] += 1 where the simplex lies wholly below En[i] (STATES).
template <bool STATES, bool CORR, int NE>
__device__ __forceinline__ void nodew_simplex3(double e0, double ea, double eb, double ec, const double (&En)[NE], double (&acc)[NE],
                                               int (&full)[NE]) {
    double e1 = e0, e2 = ea, e3 = eb, e4 = ec;
    bool o1 = true, o2 = false, o3 = false, o4 = false;
    nodew_cx(e1, e2, o1, o2);
    nodew_cx(e3, e4, o3, o4);
    nodew_cx(e1, e3, o1, o3);
    nodew_cx(e2, e4, o2, o4);
    nodew_cx(e2, e3, o2, o3);
    bool inside = false;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        inside = inside || (En[i] >= e1 && En[i] < e4);
        if (STATES && !(En[i] < e4)) ++full[i];
    }
    if (!inside) return;
    // an unselected region may have zero width: its reciprocal is then inf and never read
    const double r21 = 1.0 / (e2 - e1), r31 = 1.0 / (e3 - e1), r41 = 1.0 / (e4 - e1), r32 = 1.0 / (e3 - e2), r42 = 1.0 / (e4 - e2),
                 r43 = 1.0 / (e4 - e3);
    [[maybe_unused]] const double kap = CORR ? 0.025 * (((e1 + e2) + (e3 + e4)) - 4.0 * e0) : 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const double E = En[i];
        if (!(E >= e1 && E < e4)) continue;
        double w1, w2, w3, w4;
        double gT = 0.0;  // CORR only: the simplex's own g(E), unit = one simplex
        if (E < e2) {
            const double x = E - e1, t2 = x * r21, t3 = x * r31, t4 = x * r41;
            const double q = STATES ? 0.25 * (t2 * t3 * t4) : t3 * t4 * r21;
            if constexpr (CORR) gT = 3.0 * (t3 * t4 * r21);
            w2 = q * t2;
            w3 = q * t3;
            w4 = q * t4;
            w1 = (STATES ? 4.0 : 3.0) * q - (w2 + w3 + w4);
        } else if (E < e3) {
            const double x1 = E - e1, x2 = E - e2;
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
            const double y = e4 - E, s1 = y * r41, s2 = y * r42, s3 = y * r43;
            const double q = STATES ? 0.25 * (s1 * s2 * s3) : s1 * s2 * r43;
            if constexpr (CORR) gT = 3.0 * (s1 * s2 * r43);
            const double u1 = q * s1, u2 = q * s2, u3 = q * s3, u4 = (STATES ? 4.0 : 3.0) * q - (u1 + u2 + u3);
            w1 = STATES ? 0.25 - u1 : u1;
            w2 = STATES ? 0.25 - u2 : u2;
            w3 = STATES ? 0.25 - u3 : u3;
            w4 = STATES ? 0.25 - u4 : u4;
        }
        double f = o1 ? w1 : (o2 ? w2 : (o3 ? w3 : w4));
        if constexpr (CORR) f += gT * kap;
        acc[i] += f;
    }
}

template <bool STATES, bool CORR, int NE>
__device__ __forceinline__ void nodew_simplex2(double e0, double ea, double eb, const double (&En)[NE], double (&acc)[NE], int (&full)[NE]) {
    double e1 = e0, e2 = ea, e3 = eb;
    bool o1 = true, o2 = false, o3 = false;
    nodew_cx(e1, e2, o1, o2);
    nodew_cx(e2, e3, o2, o3);
    nodew_cx(e1, e2, o1, o2);
    constexpr double third = 1.0 / 3.0;
    bool inside = false;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        inside = inside || (En[i] >= e1 && En[i] < e3);
        if (STATES && !(En[i] < e3)) ++full[i];
    }
    if (!inside) return;
    const double r21 = 1.0 / (e2 - e1), r31 = 1.0 / (e3 - e1), r32 = 1.0 / (e3 - e2);
    [[maybe_unused]] const double kap = CORR ? (1.0 / 24.0) * (((e1 + e2) + e3) - 3.0 * e0) : 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const double E = En[i];
        if (!(E >= e1 && E < e3)) continue;
        double w1, w2, w3;
        double gT = 0.0;  // CORR only
        if (E < e2) {
            const double x = E - e1, t2 = x * r21, t3 = x * r31;
            const double q = STATES ? third * (t2 * t3) : t3 * r21;
            if constexpr (CORR) gT = 2.0 * (t3 * r21);
            w2 = q * t2;
            w3 = q * t3;
            w1 = (STATES ? 3.0 : 2.0) * q - (w2 + w3);
        } else {
            const double y = e3 - E, s1 = y * r31, s2 = y * r32;
            const double q = STATES ? third * (s1 * s2) : s1 * r32;
            if constexpr (CORR) gT = 2.0 * (s1 * r32);
            const double u1 = q * s1, u2 = q * s2, u3 = (STATES ? 3.0 : 2.0) * q - (u1 + u2);
            w1 = STATES ? third - u1 : u1;
            w2 = STATES ? third - u2 : u2;
            w3 = STATES ? third - u3 : u3;
        }
        double f = o1 ? w1 : (o2 ? w2 : w3);
        if constexpr (CORR) f += gT * kap;
        acc[i] += f;
    }
}

template <bool STATES, bool CORR, int NE>
__device__ __forceinline__ void nodew_simplex1(double e0, double ea, const double (&En)[NE], double (&acc)[NE], int (&full)[NE]) {
    double e1 = e0, e2 = ea;
    bool o1 = true, o2 = false;
    nodew_cx(e1, e2, o1, o2);
    bool inside = false;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        inside = inside || (En[i] >= e1 && En[i] < e2);
        if (STATES && !(En[i] < e2)) ++full[i];
    }
    if (!inside) return;
    const double r21 = 1.0 / (e2 - e1);
    // CORR: g_T = r21 at every energy of the window
    [[maybe_unused]] const double kap = CORR ? (1.0 / 12.0) * ((e1 + e2) - 2.0 * e0) * r21 : 0.0;
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        const double E = En[i];
        if (!(E >= e1 && E < e2)) continue;
        const double t = (E - e1) * r21;
        const double w2 = STATES ? 0.5 * t * t : t * r21, w1 = STATES ? t - w2 : r21 - w2;
        double f = o1 ? w1 : w2;
        if constexpr (CORR) f += kap;
        acc[i] += f;
    }
}

// One thread per (column of a padded grid line, band = blockIdx.y): thread t of the launch is column t % row of line t / row, so a
// wave's loads and stores are runs of consecutive columns; columns npt .. row-1 write the zeros of the padding.
template <int D, int WHAT, int NE>
__global__ __launch_bounds__(256) void ltm_nodew_kernel(NodeWArgs a) {
    constexpr bool STATES = WHAT != ABZ_LTM_DOS, CORR = WHAT == ABZ_LTM_STATES_CORRECTED;
    const int row = a.W.row, npt = a.npt;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t <= 0xffffffffll ? (int64_t)((uint32_t)t / (uint32_t)row) : t / row;
    const int i1 = (int)(t - line * row);
    double* __restrict__ const out = a.W.base + line * a.W.tile + (int64_t)(a.plane0 + (int)blockIdx.y) * a.W.pitch + i1;
    const int64_t wstep = (int64_t)a.n * a.W.pitch;  // from an energy's plane of this band to the next energy's
    if (i1 >= npt) {
#pragma unroll
        for (int i = 0; i < NE; ++i) out[i * wstep] = 0.0;
        return;
    }
    const int i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
    const int i2 = (int)line - i3 * npt;
    const int64_t tileE = a.E.tile;
    // the node's own eigenvalue, and per axis the offset to the neighbour at +1 and at -1 (every index wraps by itself)
    const double* __restrict__ const own = a.E.base + (int64_t)blockIdx.y * a.E.pitch + line * tileE + i1;
    const int64_t p0 = i1 + 1 == npt ? -(int64_t)(npt - 1) : 1, m0 = i1 == 0 ? (int64_t)(npt - 1) : -1;
    [[maybe_unused]] const int64_t p1 = (i2 + 1 == npt ? -(int64_t)(npt - 1) : 1) * tileE, m1 = (i2 == 0 ? (int64_t)(npt - 1) : -1) * tileE;
    [[maybe_unused]] const int64_t p2 = (i3 + 1 == npt ? -(int64_t)(npt - 1) : 1) * npt * tileE,
                                   m2 = (i3 == 0 ? (int64_t)(npt - 1) : -1) * npt * tileE;
    const double e0 = own[0];
    double En[NE], acc[NE];
    int full[NE];
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        En[i] = a.Es[i];
        acc[i] = 0.0;
        full[i] = 0;
    }
    // The window of the neighbourhood first: 3^d loads (a superset of the simplices' corners) against the 3 d! (d+1) loads and
    // (d+1)! sorts below.  With no energy of the group inside it every simplex lies wholly below or wholly above each energy, and
    // the node's weights are the ones the walk would give, to the bit: d! simplices' worth, or exactly 0.  Away from the surfaces
    // e = E whole waves leave here: with one energy that is most of the grid.
    {
        double nmin = e0, nmax = e0;
#pragma unroll
        for (int c = 0; c < (D == 3 ? 3 : 1); ++c) {
            const int64_t o2 = D == 3 ? (c == 0 ? m2 : (c == 1 ? 0 : p2)) : 0;
#pragma unroll
            for (int b = 0; b < (D >= 2 ? 3 : 1); ++b) {
                const int64_t o1 = D >= 2 ? (b == 0 ? m1 : (b == 1 ? 0 : p1)) : 0;
                const double va = own[o2 + o1 + m0], vb = own[o2 + o1 + p0];
                nmin = fmin(nmin, fmin(va, vb));
                nmax = fmax(nmax, fmax(va, vb));
                if (!((D < 2 || b == 1) && (D < 3 || c == 1))) {  // (the centre of the middle column is e0 itself)
                    const double vc = own[o2 + o1];
                    nmin = fmin(nmin, vc);
                    nmax = fmax(nmax, vc);
                }
            }
        }
        bool inside = false;
#pragma unroll
        for (int i = 0; i < NE; ++i) inside = inside || (En[i] >= nmin && En[i] < nmax);
        if (!inside) {
            constexpr double whole = D == 3 ? 6.0 : (D == 2 ? 2.0 : 1.0);  // (d+1)! simplices of 1 / (d+1) each
#pragma unroll
            for (int i = 0; i < NE; ++i) out[i * wstep] = STATES && !(En[i] < nmax) ? a.weight * whole : 0.0;
            return;
        }
    }
    if constexpr (D == 3) {
        // the permutation (X, Y, Z) of the axes; a loop, the axes' offsets by selects
#pragma unroll 1
        for (int s = 0; s < 6; ++s) {
            const int X = s >> 1, Y = (X + 1 + (s & 1)) % 3, Z = 3 - X - Y;
            const int64_t pX = X == 0 ? p0 : (X == 1 ? p1 : p2), mX = X == 0 ? m0 : (X == 1 ? m1 : m2);
            const int64_t pY = Y == 0 ? p0 : (Y == 1 ? p1 : p2), mY = Y == 0 ? m0 : (Y == 1 ? m1 : m2);
            const int64_t pZ = Z == 0 ? p0 : (Z == 1 ? p1 : p2), mZ = Z == 0 ? m0 : (Z == 1 ? m1 : m2);
            nodew_simplex3<STATES, CORR, NE>(e0, own[pX], own[pX + pY], own[pX + pY + pZ], En, acc, full);
            nodew_simplex3<STATES, CORR, NE>(e0, own[mX], own[pY], own[pY + pZ], En, acc, full);
            nodew_simplex3<STATES, CORR, NE>(e0, own[mX + mY], own[mY], own[pZ], En, acc, full);
            nodew_simplex3<STATES, CORR, NE>(e0, own[mX + mY + mZ], own[mY + mZ], own[mZ], En, acc, full);
        }
    } else if constexpr (D == 2) {
#pragma unroll 1
        for (int s = 0; s < 2; ++s) {
            const int64_t pX = s == 0 ? p0 : p1, mX = s == 0 ? m0 : m1;
            const int64_t pY = s == 0 ? p1 : p0, mY = s == 0 ? m1 : m0;
            nodew_simplex2<STATES, CORR, NE>(e0, own[pX], own[pX + pY], En, acc, full);
            nodew_simplex2<STATES, CORR, NE>(e0, own[mX], own[pY], En, acc, full);
            nodew_simplex2<STATES, CORR, NE>(e0, own[mX + mY], own[mY], En, acc, full);
        }
    } else {
        nodew_simplex1<STATES, CORR, NE>(e0, own[p0], En, acc, full);
        nodew_simplex1<STATES, CORR, NE>(e0, own[m0], En, acc, full);
    }
#pragma unroll
    for (int i = 0; i < NE; ++i) {
        // the simplices wholly below E: an integer count, divided once (exact for the (d+1)! of a full neighbourhood)
        const double v = STATES ? acc[i] + (double)full[i] / (double)(D + 1) : acc[i];
        out[i * wstep] = a.weight * v;
    }
}

using NodeWFn = void (*)(NodeWArgs);
// [d - 1][what][NE == 4]
constexpr NodeWFn LTM_NODEW[3][3][2] = {
    {{ltm_nodew_kernel<1, ABZ_LTM_DOS, 1>, ltm_nodew_kernel<1, ABZ_LTM_DOS, 4>},
     {ltm_nodew_kernel<1, ABZ_LTM_STATES, 1>, ltm_nodew_kernel<1, ABZ_LTM_STATES, 4>},
     {ltm_nodew_kernel<1, ABZ_LTM_STATES_CORRECTED, 1>, ltm_nodew_kernel<1, ABZ_LTM_STATES_CORRECTED, 4>}},
    {{ltm_nodew_kernel<2, ABZ_LTM_DOS, 1>, ltm_nodew_kernel<2, ABZ_LTM_DOS, 4>},
     {ltm_nodew_kernel<2, ABZ_LTM_STATES, 1>, ltm_nodew_kernel<2, ABZ_LTM_STATES, 4>},
     {ltm_nodew_kernel<2, ABZ_LTM_STATES_CORRECTED, 1>, ltm_nodew_kernel<2, ABZ_LTM_STATES_CORRECTED, 4>}},
    {{ltm_nodew_kernel<3, ABZ_LTM_DOS, 1>, ltm_nodew_kernel<3, ABZ_LTM_DOS, 4>},
     {ltm_nodew_kernel<3, ABZ_LTM_STATES, 1>, ltm_nodew_kernel<3, ABZ_LTM_STATES, 4>},
     {ltm_nodew_kernel<3, ABZ_LTM_STATES_CORRECTED, 1>, ltm_nodew_kernel<3, ABZ_LTM_STATES_CORRECTED, 4>}},
};
static_assert(ABZ_LTM_DOS == 0 && ABZ_LTM_STATES == 1 && ABZ_LTM_STATES_CORRECTED == 2, "the table's middle index is `what`");

// ---------------------------------------------------------------------------------------------------------------------
// Dot: sum_k sum_b w_b(k; E_i) A_{c,b}(k)
// ---------------------------------------------------------------------------------------------------------------------
// blockIdx.y = energy; a thread walks (line, band, column) triples of the block's share in a fixed stride, consecutive threads
// consecutive columns, and contracts the weight it loaded with every component.  (A variant that gave a block whole rows -- no
// division per element, idle threads where 256 is no multiple of the row -- was measured 1.4 times slower at 150^3 and 48^3.)
// partial [nE ncomp][nrows], column iE ncomp + c, row blockIdx.x.
__global__ __launch_bounds__(256) void ltm_nodew_dot_kernel(PlaneView W, PlaneView A, int n, int npt, int ncomp, int64_t nlines,
                                                            double* __restrict__ partial, int64_t nrows) {
    __shared__ double red[4][ABZ_LTM_MAX_COMP];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int row = W.row;
    const int64_t total = nlines * n * row;
    const double* __restrict__ const Wb = W.base + (int64_t)blockIdx.y * n * W.pitch;
    const int64_t acomp = (int64_t)n * A.pitch;
    double acc[ABZ_LTM_MAX_COMP];
#pragma unroll
    for (int c = 0; c < ABZ_LTM_MAX_COMP; ++c) acc[c] = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (int64_t)gridDim.x * 256) {
        const int64_t lb = t <= 0xffffffffll ? (int64_t)((uint32_t)t / (uint32_t)row) : t / row;
        const int i1 = (int)(t - lb * row);
        if (i1 >= npt) continue;  // (the weights of the padding are zero; its elements need not be finite)
        const int64_t line = lb / n;
        const int b = (int)(lb - line * n);
        const double w = Wb[line * W.tile + (int64_t)b * W.pitch + i1];
        const double* __restrict__ const Ap = A.base + line * A.tile + (int64_t)b * A.pitch + i1;
#pragma unroll
        for (int c = 0; c < ABZ_LTM_MAX_COMP; ++c)
            if (c < ncomp) acc[c] += w * Ap[c * acomp];
    }
    // every lane ends with the same bits: a + b == b + a at every level of the butterfly
#pragma unroll
    for (int c = 0; c < ABZ_LTM_MAX_COMP; ++c) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc[c] += __shfl_xor(acc[c], off);
        if (lane == 0) red[wave][c] = acc[c];
    }
    __syncthreads();
    if ((int)threadIdx.x < ncomp) {
        const int c = (int)threadIdx.x;
        partial[((int64_t)blockIdx.y * ncomp + c) * nrows + blockIdx.x] = (red[0][c] + red[1][c]) + (red[2][c] + red[3][c]);
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// Fold: the weights of an unfolded rule summed over each orbit onto the source rule's nodes
// ---------------------------------------------------------------------------------------------------------------------
// start [nirr + 1], member [npt^d]: the grid points of node j's orbit are member[start[j] .. start[j + 1]), ascending.
// out [nE][nirr][n]; thread t = (iE nirr + j) n + b.
__global__ __launch_bounds__(256) void ltm_nodew_fold_kernel(PlaneView W, const int64_t* __restrict__ start, const int32_t* __restrict__ member,
                                                             int n, int nE, int64_t nirr, double* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= (int64_t)nE * nirr * n) return;
    const int64_t ej = t / n;
    const int b = (int)(t - ej * n);
    const int64_t iE = ej / nirr, j = ej - iE * nirr;
    const double* __restrict__ const Wp = W.base + ((int64_t)iE * n + b) * W.pitch;
    double s = 0.0;
    for (int64_t m = start[j]; m < start[j + 1]; ++m) {
        const int64_t k = member[m];
        const int64_t line = k / W.line_len;
        s += Wp[line * W.tile + (k - line * W.line_len)];
    }
    out[t] = s;
}

}  // namespace

// The block W (nE n planes, tiled like the eigenvalue planes E with pitch = row, padding columns included) <- w_b(k; Es[i]).
// Launches only; groups of 4 energies, then single ones.
int launch_ltm_node_weights(abz_ctx* ctx, int n, int d, int npt, PlaneView E, PlaneView W, const double* Es_host, int nE, int what) {
    NodeWArgs a;
    a.E = E;
    a.W = W;
    a.npt = npt;
    a.n = n;
    a.nlines = 1;
    for (int j = 1; j < d; ++j) a.nlines *= npt;
    a.weight = 1.0 / ((double)(d == 3 ? 6 : (d == 2 ? 2 : 1)) * (double)(a.nlines * npt));
    const dim3 grid((unsigned)cdiv64(a.nlines * W.row, 256), (unsigned)n);
    ProfScope ps(ctx, ABZ_K_LTM);
    for (int i0 = 0; i0 < nE;) {
        const int ne = nE - i0 >= 4 ? 4 : 1;
        for (int i = 0; i < 4; ++i) a.Es[i] = Es_host[i0 + std::min(i, ne - 1)];
        a.plane0 = i0 * n;
        launch(ctx, LTM_NODEW[d - 1][what][ne == 4], grid, dim3(256), 0, a);
        ABZ_HIP(hipGetLastError());
        i0 += ne;
    }
    return ABZ_OK;
}

// out_host [nE][ncomp] = sum_k sum_b W A; one synchronisation
int launch_ltm_node_weights_dot(abz_ctx* ctx, int n, int npt, int64_t nlines, PlaneView W, int nE, PlaneView A, int ncomp, double* out_host) {
    const int64_t total = nlines * n * W.row;
    const int64_t nblocks = std::max<int64_t>(1, std::min<int64_t>(cdiv64(total, 256), std::max(64, 2048 / nE)));
    const int ncol = nE * ncomp;
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)nblocks * (size_t)ncol);
    if (rc) return rc;
    double* partial = ctx->scratch[1].as<double>();
    // the columns travel as pairs of doubles: the mailbox and its fallback speak double2
    const int64_t npair = (ncol + 1) / 2;
    std::vector<double> pairs(2 * (size_t)npair);
    const SumOut so = sum_out_mailbox(ctx, pairs.data(), (size_t)npair);
    double2* where = nullptr;
    if ((rc = sum_target(ctx, so, 0, npair, &where))) return rc;
    {
        ProfScope ps(ctx, ABZ_K_LTM);
        launch(ctx, ltm_nodew_dot_kernel, dim3((unsigned)nblocks, (unsigned)nE), dim3(256), 0, W, A, n, npt, ncomp, nlines, partial, nblocks);
        ABZ_HIP(hipGetLastError());
        // column by column as they are (scale 1: x to the bit)
        if ((rc = launch_ltm_final(ctx, partial, nblocks, 1.0, ncol, ncol, 0, reinterpret_cast<double*>(where)))) return rc;
    }
    if ((rc = sum_deliver(ctx, so, where, 0, npair))) return rc;
    std::memcpy(out_host, pairs.data(), sizeof(double) * (size_t)ncol);
    return ABZ_OK;
}

// The inverse of an orbit map on the host: node_of [N] (every entry inside 0 .. nirr-1) -> start [nirr + 1], member [N] with the
// points of every orbit ascending (a counting sort).
void ltm_orbit_inverse(const int32_t* node_of, int64_t N, int64_t nirr, std::vector<int64_t>& start, std::vector<int32_t>& member) {
    start.assign((size_t)nirr + 1, 0);
    for (int64_t x = 0; x < N; ++x) start[(size_t)node_of[x] + 1] += 1;
    for (int64_t j = 0; j < nirr; ++j) start[(size_t)j + 1] += start[(size_t)j];
    member.resize((size_t)N);
    std::vector<int64_t> fill(start.begin(), start.end() - 1);
    for (int64_t x = 0; x < N; ++x) member[(size_t)fill[(size_t)node_of[x]]++] = (int32_t)x;
}

// out_dev [nE][nirr][n] <- the orbit sums of W.  Launches only.
int launch_ltm_node_weights_fold(abz_ctx* ctx, int n, PlaneView W, int nE, const int64_t* start, const int32_t* member, int64_t nirr,
                                 double* out_dev) {
    const int64_t total = (int64_t)nE * nirr * n;
    ProfScope ps(ctx, ABZ_K_LTM);
    launch(ctx, ltm_nodew_fold_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, W, start, member, n, nE, nirr, out_dev);
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
