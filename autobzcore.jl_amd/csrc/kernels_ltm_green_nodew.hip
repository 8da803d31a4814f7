// Linear tetrahedron method (gfx950 only): the complex integration weights W_b(k; z) of the Green's function per grid point and
// band, in gather form -- the complex sibling of ltm_nodew_kernel (kernels_ltm_nodew.hip).
//
// The scans of kernels_ltm_green.hip form the corner weights W_i(z) of every simplex and contract them at once with what is
// attached.  Here the weights themselves are the result: the numbers with
//      G_A(z) = sum_k sum_b W_b(k; z) A_b(k)
// for ANY A (complex, matrix-valued, or not known when the weights are made), as a resident block tiled like the eigenvalue
// planes: plane (2 i + part) n + b of a grid line's tile is Re (part 0) or Im (part 1) of the weight of band b at z_i, pitch
// E.row, padding columns zero.  Every consumer of a real weight block (the dot, the fold, the density-matrix contraction) reads
// it as 2 nz real weight sets.
//
//  * Quantity.  W_b(k; z) = w sum_{T contains k} W^T_{i(k)}(z), w = 1 / (d! npt^d), over the (d+1)! Kuhn simplices that contain
//    node k: the geometry of ltm_nodew_kernel (every permutation of the axes, every position of k in the chain, every index
//    wrapped mod npt, npt = 2 included).  W^T_i(z) = J[x_0 .. x_m, x_i](z) / (m + 1) is the corner weight of the weighted scan,
//    formed by the very device functions of that scan (ltm_green_device.h: green_weights<NK> with its evaluation rule, rho = 1/2,
//    the Taylor series for narrow sub-ranges, the principal logs of one half plane and the "all multisets narrow" shortcut).
//  * Own corner.  The sort of a simplex carries a one-hot flag "this corner is the node", as nodew_cx carries its flag.  Only the
//    node's own weight is needed.  Where its multiset (the sorted corners with the own knot doubled) is narrow -- a fine grid
//    away from the corners' energies: most simplices -- it is ONE Taylor series, the one green_weights would sum for that corner,
//    to the bit; neither the other m series nor a logarithm is formed.  Elsewhere green_weights forms all m + 1 weights as in the
//    scan, from corner logs taken there, and the flags select the node's (DESIGN section 4e says what forming the own multiset's
//    doubled-knot chain alone would save on that path).
//  * Shape.  One thread per (column of a padded line, band = blockIdx.y); neighbour addresses are the node's own plus one
//    precomputed offset per axis; ONE loop over (permutation, position) that is not unrolled, its offsets by selects, so the
//    weight routine is inlined once per value of z; no register array is indexed at run time (the sorted position of the node
//    selects knots, it indexes nothing).  The NZ = 1 or 2 values of z of a launch go by value and share the loads and the sort
//    (pairs in one and two variables only: green_nodew_nz).
//  * No atomics: a thread sums its simplices in program order, the launch geometry depends on (n, npt, d, nz) alone and two
//    calls write the same bits.  Im z < 0: computed at conj(z) and conjugated at the store, so the value is the conjugate of the
//    one at conj(z) to the bit.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_green_device.h"

namespace abz {

namespace {

struct GreenNodeWArgs {
    PlaneView E, W;   // eigenvalue planes; the weight block (2 nz n planes per tile, pitch = row)
    int64_t nlines;   // npt^(d-1)
    int npt;
    int plane0;       // first weight plane of this launch: 2 (its first z) n
    int n;
    double weight;    // 1 / (d! npt^d (d+1)): of a simplex, and of its corner weights the 1 / (m + 1)
    double z[2][2];   // the launch's values of z (NZ of them): re, im of either sign
};

// what the sort of a simplex carries per corner: the energy and "this corner is the node itself"
struct GreenNodeCorner {
    double x;
    bool own;
};

__device__ __forceinline__ void gnw_cx(GreenNodeCorner& a, GreenNodeCorner& b) {
    const bool sw = b.x < a.x;
    const double lo = sw ? b.x : a.x, hi = sw ? a.x : b.x;
    const bool x = sw ? b.own : a.own, y = sw ? a.own : b.own;
    a = {lo, x};
    b = {hi, y};
}

// One simplex: the node's own corner and its NK - 1 other corners in any order.  (accr, acci)[i] += (m + 1) times the weight the
// simplex gives the node at z_i, i.e. J of the sorted corners with the node's own knot doubled.  green_weights would return it as
// one of its m + 1 weights; where the own multiset is narrow -- a fine grid away from the corners' energies: most simplices -- that
// weight is the Taylor series of its m + 2 knots alone (green_node takes this very decision from these very numbers, and the
// series is the one green_weights sums: the same bits), so neither the other m series nor a corner's logarithm is formed.
// Elsewhere all m + 1 weights are formed as in the scan and the flags select the node's.
template <int NK, int NZ>
__device__ __forceinline__ void gnw_simplex(GreenNodeCorner (&q)[NK], const double (&zr)[NZ], const double (&zi)[NZ], double (&accr)[NZ],
                                            double (&acci)[NZ]) {
    if constexpr (NK == 2) {
        gnw_cx(q[0], q[1]);
    } else if constexpr (NK == 3) {
        gnw_cx(q[0], q[1]);
        gnw_cx(q[1], q[2]);
        gnw_cx(q[0], q[1]);
    } else {
        gnw_cx(q[0], q[1]);
        gnw_cx(q[2], q[3]);
        gnw_cx(q[0], q[2]);
        gnw_cx(q[1], q[3]);
        gnw_cx(q[1], q[2]);
    }
    // the sorted position of the node
    int pos = NK - 1;
#pragma unroll
    for (int l = NK - 2; l >= 0; --l) pos = q[l].own ? l : pos;
    const double w = q[NK - 1].x - q[0].x;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        // u of the own multiset x_0 .. x_pos, x_pos .. x_m: knot l is corner l up to the node, corner l - 1 behind it
        double uu[NK + 1];
        uu[0] = zr[i] - q[0].x;
        uu[NK] = zr[i] - q[NK - 1].x;
#pragma unroll
        for (int l = 1; l < NK; ++l) uu[l] = zr[i] - (pos >= l ? q[l].x : q[l - 1].x);
        const double ur = green_mean<NK>(uu), n2 = ur * ur + zi[i] * zi[i];
        Cx f;
        if (w * w < GREEN_RHO2 * n2) {
            f = green_series<NK>(uu, ur, zi[i], n2);
        } else {
            GreenCorner g[NK];
#pragma unroll
            for (int l = 0; l < NK; ++l) {
                const double u = zr[i] - q[l].x;
                g[l] = {q[l].x, 0.5 * log(u * u + zi[i] * zi[i]), atan2(zi[i], u)};
            }
            Cx W[NK];
            green_weights<NK>(g, zr[i], zi[i], W);
            f = W[NK - 1];
#pragma unroll
            for (int l = NK - 2; l >= 0; --l) {
                f.re = q[l].own ? W[l].re : f.re;
                f.im = q[l].own ? W[l].im : f.im;
            }
        }
        accr[i] += f.re;
        acci[i] += f.im;
    }
}

// One thread per (column of a padded grid line, band = blockIdx.y), as ltm_nodew_kernel: thread t of the launch is column t % row
// of line t / row; columns npt .. row-1 write the zeros of the padding.
template <int D, int NZ>
__global__ __launch_bounds__(256) void ltm_green_nodew_kernel(GreenNodeWArgs a) {
    const int row = a.W.row, npt = a.npt;
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= a.nlines * row) return;
    const int64_t line = t <= 0xffffffffll ? (int64_t)((uint32_t)t / (uint32_t)row) : t / row;
    const int i1 = (int)(t - line * row);
    double* __restrict__ const out = a.W.base + line * a.W.tile + (int64_t)(a.plane0 + (int)blockIdx.y) * a.W.pitch + i1;
    const int64_t wstep = (int64_t)a.n * a.W.pitch;  // from a plane of this band to the next part's / the next z's
    if (i1 >= npt) {
#pragma unroll
        for (int i = 0; i < 2 * NZ; ++i) out[i * wstep] = 0.0;
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
    double zr[NZ], zi[NZ], accr[NZ], acci[NZ];
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        zr[i] = a.z[i][0];
        zi[i] = fabs(a.z[i][1]);
        accr[i] = 0.0;
        acci[i] = 0.0;
    }
    const GreenNodeCorner c0 = {own[0], true};
    if constexpr (D == 3) {
        // (permutation (X, Y, Z) of the axes, position j of the node in the chain): the simplices of ltm_nodew_kernel in one loop
#pragma unroll 1
        for (int sj = 0; sj < 24; ++sj) {
            const int s = sj >> 2, j = sj & 3;
            const int X = s >> 1, Y = (X + 1 + (s & 1)) % 3, Z = 3 - X - Y;
            const int64_t pX = X == 0 ? p0 : (X == 1 ? p1 : p2), mX = X == 0 ? m0 : (X == 1 ? m1 : m2);
            const int64_t pY = Y == 0 ? p0 : (Y == 1 ? p1 : p2), mY = Y == 0 ? m0 : (Y == 1 ? m1 : m2);
            const int64_t pZ = Z == 0 ? p0 : (Z == 1 ? p1 : p2), mZ = Z == 0 ? m0 : (Z == 1 ? m1 : m2);
            // j = 0: k, k+X, k+X+Y, k+X+Y+Z   1: k-X, k, k+Y, k+Y+Z   2: k-X-Y, k-Y, k, k+Z   3: k-X-Y-Z, k-Y-Z, k-Z, k
            const int64_t oa = j == 0 ? pX : (j == 1 ? mX : (j == 2 ? mX + mY : mX + mY + mZ));
            const int64_t ob = j == 0 ? pX + pY : (j == 1 ? pY : (j == 2 ? mY : mY + mZ));
            const int64_t oc = j == 0 ? pX + pY + pZ : (j == 1 ? pY + pZ : (j == 2 ? pZ : mZ));
            GreenNodeCorner q[4] = {c0, {own[oa], false}, {own[ob], false}, {own[oc], false}};
            gnw_simplex<4, NZ>(q, zr, zi, accr, acci);
        }
    } else if constexpr (D == 2) {
#pragma unroll 1
        for (int sj = 0; sj < 6; ++sj) {
            const int s = sj >= 3 ? 1 : 0, j = sj - 3 * s;
            const int64_t pX = s == 0 ? p0 : p1, mX = s == 0 ? m0 : m1;
            const int64_t pY = s == 0 ? p1 : p0, mY = s == 0 ? m1 : m0;
            // j = 0: k, k+X, k+X+Y   1: k-X, k, k+Y   2: k-X-Y, k-Y, k
            const int64_t oa = j == 0 ? pX : (j == 1 ? mX : mX + mY);
            const int64_t ob = j == 0 ? pX + pY : (j == 1 ? pY : mY);
            GreenNodeCorner q[3] = {c0, {own[oa], false}, {own[ob], false}};
            gnw_simplex<3, NZ>(q, zr, zi, accr, acci);
        }
    } else {
#pragma unroll 1
        for (int j = 0; j < 2; ++j) {
            GreenNodeCorner q[2] = {c0, {own[j == 0 ? p0 : m0], false}};
            gnw_simplex<2, NZ>(q, zr, zi, accr, acci);
        }
    }
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
        const double re = a.weight * accr[i], im = a.weight * acci[i];
        out[(2 * i) * wstep] = re;
        out[(2 * i + 1) * wstep] = a.z[i][1] < 0.0 ? -im : im;
    }
}

// Values of z per launch where at least that many remain: 2 in one and two variables (the pair shares the loads and the sort), 1 in
// three, where the pair's instantiation needs every VGPR and 4 AGPRs, runs one wave per SIMD and was measured slower per z than
// two launches of one.
constexpr int green_nodew_nz(int d) { return d == 3 ? 1 : 2; }

using GreenNodeWFn = void (*)(GreenNodeWArgs);
// [d - 1][NZ == 2]
constexpr GreenNodeWFn LTM_GREEN_NODEW[3][2] = {
    {ltm_green_nodew_kernel<1, 1>, ltm_green_nodew_kernel<1, 2>},
    {ltm_green_nodew_kernel<2, 1>, ltm_green_nodew_kernel<2, 2>},
    {ltm_green_nodew_kernel<3, 1>, nullptr},
};
static_assert(green_nodew_nz(3) == 1, "no pair kernel in three variables");

}  // namespace

// The block W (2 nz n planes, tiled like the eigenvalue planes E with pitch = row, padding columns included) <- W_b(k; z_i),
// z_host [nz][2] with Im z != 0.  Launches only; groups of green_nodew_nz(d) values, then single ones.
int launch_ltm_green_node_weights(abz_ctx* ctx, int n, int d, int npt, PlaneView E, PlaneView W, const double* z_host, int nz) {
    GreenNodeWArgs a;
    a.E = E;
    a.W = W;
    a.npt = npt;
    a.n = n;
    a.nlines = 1;
    for (int j = 1; j < d; ++j) a.nlines *= npt;
    a.weight = 1.0 / ((double)ltm_nsimplex(d) * (double)(a.nlines * npt) * (double)(d + 1));
    const dim3 grid((unsigned)cdiv64(a.nlines * W.row, 256), (unsigned)n);
    ProfScope ps(ctx, ABZ_K_LTM);
    for (int i0 = 0; i0 < nz;) {
        const int cnt = nz - i0 >= green_nodew_nz(d) ? green_nodew_nz(d) : 1;
        for (int i = 0; i < 2; ++i) {
            const int k = i0 + std::min(i, cnt - 1);
            a.z[i][0] = z_host[2 * k];
            a.z[i][1] = z_host[2 * k + 1];
        }
        a.plane0 = 2 * i0 * n;
        launch(ctx, LTM_GREEN_NODEW[d - 1][cnt == 2], grid, dim3(256), 0, a);
        ABZ_HIP(hipGetLastError());
        i0 += cnt;
    }
    return ABZ_OK;
}

}  // namespace abz
