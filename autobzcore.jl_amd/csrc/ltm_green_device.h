// What the tetrahedron Green's-function files share (kernels_ltm_green.hip, kernels_ltm_green_nodew.hip, kernels_ltm_green_opt.hip):
// the evaluation rule of J[x_0 .. x_m](z) -- the Taylor series of a narrow sub-range, the pair from the corner logs, the recursion
// of a wide one --, the J of a whole simplex (the trace), the corner weights (m + 1) W_i = J[x_0 .. x_m, x_i] of a sorted simplex,
// the sort that carries NC elements per corner and contracts them with the weights, and the values of z a launch takes.
// kernels_ltm_green.hip has the derivation and the bounds; everything here is inlined into the kernels of the file that includes it.
#pragma once

#include <hip/hip_runtime.h>

#include <type_traits>

#include "ltm_device.h"

namespace abz {

namespace {

constexpr double GREEN_RHO2 = 0.25;      // rho^2
constexpr double GREEN_EPS2 = 0x1p-104;  // (2^-52)^2
constexpr int GREEN_KMAX = 40;           // terms beyond k = 37 (the five knots of a corner weight: 39) are never asked for

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

// values of z per launch (kernels_ltm_green.hip has the LDS layout): the trace, then a group of NC components
constexpr int LTM_GREEN_CHUNK = 512;     // values of z per launch: 8 (2 + 4 x 2) B of LDS each
static_assert(sizeof(double) * 10 * LTM_GREEN_CHUNK <= LTM_LDS_MAX, "the z list and the four waves' sums fit the scans' LDS");
constexpr int green_w_chunk(int nc) {
    const size_t fit = LTM_LDS_MAX / (sizeof(double) * (size_t)(2 + 8 * nc));
    return fit < (size_t)LTM_GREEN_CHUNK ? (int)fit : LTM_GREEN_CHUNK;
}
static_assert(sizeof(double) * (2 + 8 * 1) * green_w_chunk(1) <= LTM_LDS_MAX && sizeof(double) * (2 + 8 * 2) * green_w_chunk(2) <= LTM_LDS_MAX &&
                  sizeof(double) * (2 + 8 * 4) * green_w_chunk(4) <= LTM_LDS_MAX,
              "the z list and the four waves' sums of every component group fit the scans' LDS");
static_assert(green_w_chunk(1) == LTM_GREEN_CHUNK, "the trace is a group of one component");
static_assert(green_w_chunk(4) >= 4 && green_w_chunk(4) <= green_w_chunk(2) && green_w_chunk(2) <= green_w_chunk(1), "chunks shrink with NC");

// what the sort of a simplex carries per corner: the energy, log(z - energy) and the NC elements
template <int NC>
struct GreenWCorner {
    GreenCorner g;
    LtmVec<NC> a;
};
template <int NC>
__device__ __forceinline__ GreenWCorner<NC> green_sel(bool first, const GreenWCorner<NC>& p, const GreenWCorner<NC>& q) {
    GreenWCorner<NC> r;
    r.g = green_sel(first, p.g, q.g);
#pragma unroll
    for (int c = 0; c < NC; ++c) r.a.v[c] = first ? p.a.v[c] : q.a.v[c];
    return r;
}
template <int NC>
__device__ __forceinline__ void green_wcx(GreenWCorner<NC>& p, GreenWCorner<NC>& q) {
    const bool sw = q.g.x < p.g.x;
    const GreenWCorner<NC> lo = green_sel(sw, q, p), hi = green_sel(sw, p, q);
    p = lo;
    q = hi;
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

}  // namespace

}  // namespace abz
