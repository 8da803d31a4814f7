// What the tetrahedron scans share (kernels_ltm.hip, kernels_ltm_pairs_occ.hip): the first energy of a window, the histogram add and
// the closed forms of one simplex with matrix elements.  The routines stood in kernels_ltm.hip and moved here verbatim when the
// occupied pair scan became a second reader; the formulas are described at the head of that file.
#pragma once

#include <hip/hip_runtime.h>

#include "ltm_device.h"

namespace abz {

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

// One tetrahedron, corners in any order.  hist / step: [NC][nE] of the wave.  P: a payload with NC and CORR (LtmElems<NC, CORR>).
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

}  // namespace abz
