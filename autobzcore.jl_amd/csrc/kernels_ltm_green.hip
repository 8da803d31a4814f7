// Linear tetrahedron method (gfx950 only): Green's functions at complex energies, tr G(z) and G_A(z), on the mesh of kernels_ltm.hip
// (its header has the geometry: the Kuhn split of the cells of a periodic grid, the simplex weight, the band convention).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <type_traits>
#include <vector>

#include "abz_internal.h"
#include "ltm_device.h"
#include "ltm_green_device.h"

namespace abz {

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// Trace of the Green's function at complex energies (abz_rule_ltm_green)
// ---------------------------------------------------------------------------------------------------------------------
// tr G(z) = w sum_{cells} sum_{d! simplices} sum_{bands} J[x_0 .. x_d](z), w = 1 / (d! npt^d), on the mesh of the window scans.
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
//  * Shape (ltm_green_kernel<D, GreenTrace>, at the end of this file).  Not a window scan: every simplex contributes at every z,
//    there is no queue and no histogram.  The cell walk and the whole-grid corner geometry are ltm_window_kernel's (ltm_cell,
//    ltm_wrap): blocks of 256 cells, one cell per thread, blockIdx.y the band, the 2^d corner energies in registers, the values
//    of z in LDS.  Per (cell, z) the 2^d complex logs of z - e_corner are taken once and shared by the cell's d! simplices; the
//    sorting network of a simplex carries each corner's log along with its energy, as LtmElems carries elements, and the pair
//    formula reads them.  blockIdx.z splits the values of z of a launch where the cells alone do not fill the device.
//  * Reduction.  Per z in a fixed order: a butterfly over the wave, lane 0 adds into the wave's LDS slot [nz][re, im] in
//    program order, the four waves are summed in a fixed order into transposed partials and launch_ltm_final finishes.  No
//    atomics: two calls return the same bits.
struct GreenArgs {
    PlaneView E;
    const double* z;  // device [nz][2]: re, im > 0
    int64_t ncell;    // npt^d
    int npt, nz;
    int zper;         // values of z per blockIdx.z
};

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
//  * Shape (ltm_green_kernel<D, GreenElems<NC>>).  The same kernel with another payload: the 2^d corner energies and the NC 2^d
//    corner elements of a group of NC components stay in registers (ltm_load through PlaneView / acomp), the sort of a simplex
//    carries each corner's log and its NC elements, the m + 1 weights of a (simplex, z) are formed once and every component
//    contracts with them.  Groups as in ltm_scan: 4s, a 2, a 1.  LDS: [zn][2] z | [4 waves][zn][NC][2] sums, so a launch takes
//    green_w_chunk(NC) = 512 / 291 / 154 values of z.  1 / (m + 1) goes into the scale of launch_ltm_final.
struct GreenWArgs : GreenArgs {
    PlaneView A;
    int64_t acomp;  // doubles from a band's plane of one component to its plane of the next: n * A.pitch
    int aplane0;    // first element plane of this launch: (its first component) * n
};

// ---------------------------------------------------------------------------------------------------------------------
// The scan: one kernel, two payloads
// ---------------------------------------------------------------------------------------------------------------------
// A payload says what a corner carries through the sort of a simplex besides its energy and its logarithm: Args is its
// kernel-argument struct, Vec what a cell keeps per corner (load), Corner what is sorted (make; green_sel picks by its type),
// simplex the routine that adds one simplex to the NC sums.  The z list, the cell walk, the geometry, the corner logs, the loop
// over the Kuhn simplices and the reduction are the kernel's and exist once.  The hooks are inlined before anything else.
// Col is the integer type in which the write-out forms its column index (at most 2 x 4 x 512: either holds it).  The two kernels
// this one replaced formed it in these two types, and the address arithmetic the compiler keeps across the whole kernel follows
// the type: with one type for both, the trace loses 2 VGPRs and 0.8 % at 150^3 (int64_t) or the components gain 2 VGPRs (int).
// With Col every instantiation keeps its instruction stream and its registers.
//
// The trace: nothing but the energy, one sum.
struct GreenTrace {
    static constexpr int NC = 1;
    using Args = GreenArgs;
    struct Vec {};
    using Corner = GreenCorner;
    static __device__ __forceinline__ Vec load(const Args&, int64_t, int) { return {}; }
    static __device__ __forceinline__ Corner make(const GreenCorner& g, const Vec&) { return g; }
    using Col = int;
    // d = 1 (NK = 2): the cell's only simplex is the sum
    template <int NK>
    static __device__ __forceinline__ void simplex(Corner (&q)[NK], double zr, double zi, double (&sr)[1], double (&si)[1]) {
        Cx J;
        if constexpr (NK == 4) J = green_simplex(q[0], q[1], q[2], q[3], zr, zi);
        else if constexpr (NK == 3) J = green_simplex(q[0], q[1], q[2], zr, zi);
        else J = green_simplex(q[0], q[1], zr, zi);
        sr[0] = NK == 2 ? J.re : sr[0] + J.re;
        si[0] = NK == 2 ? J.im : si[0] + J.im;
    }
};

// Matrix elements: NC components per corner, from the planes of the launch's first component on.
template <int NC_>
struct GreenElems {
    static constexpr int NC = NC_;
    using Args = GreenWArgs;
    using Vec = LtmVec<NC>;
    using Corner = GreenWCorner<NC>;
    // the corner at column i1 of line `line` of this band's planes
    static __device__ __forceinline__ Vec load(const Args& a, int64_t line, int i1) {
        return ltm_load<NC>(a.A.base + (int64_t)(a.aplane0 + (int)blockIdx.y) * a.A.pitch + line * a.A.tile + i1, a.acomp);
    }
    static __device__ __forceinline__ Corner make(const GreenCorner& g, const Vec& v) { return {g, v}; }
    using Col = int64_t;
    template <int NK>
    static __device__ __forceinline__ void simplex(Corner (&q)[NK], double zr, double zi, double (&sr)[NC], double (&si)[NC]) {
        green_wsimplex<NK, NC>(q, zr, zi, sr, si);
    }
};

// partial [2 NC nz][nrows]: column (i NC + c) 2 + {0, 1} the real and imaginary part of component c's sum at z_i
template <int D, class P>
__global__ __launch_bounds__(256) void ltm_green_kernel(typename P::Args a, double* __restrict__ partial, int64_t nrows) {
    // [zn][2] this block's values of z | [4 waves][zn][NC][2] sums
    extern __shared__ __attribute__((aligned(16))) double ldsg[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    constexpr int NV = 1 << D;  // corners per cell
    constexpr int NC = P::NC;
    using Corner = typename P::Corner;
    const int z0 = (int)blockIdx.z * a.zper;
    const int zn = min(a.zper, a.nz - z0);
    const double* const zl = ldsg;
    double* const acc = ldsg + (size_t)2 * zn * (1 + NC * wave);
    for (int i = threadIdx.x; i < 2 * zn; i += 256) ldsg[i] = a.z[2 * z0 + i];
    for (int i = threadIdx.x; i < 8 * NC * zn; i += 256) ldsg[2 * zn + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const double* __restrict__ const Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    const int64_t tileE = a.E.tile;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        const bool active = k < a.ncell;
        double c[NV];
        typename P::Vec ca[NV];
#pragma unroll
        for (int j = 0; j < NV; ++j) {
            c[j] = 0.0;
            ca[j] = {};
        }
        if (active) {
            const LtmCell cell = ltm_cell<D>(k, npt);
#pragma unroll
            for (int j = 0; j < NV; ++j) {
                int j1 = cell.i1, j2 = cell.i2, j3 = cell.i3;
                ltm_wrap<D>(j1, j2, j3, j, npt);
                const int64_t line = (int64_t)j3 * npt + j2;
                c[j] = Eb[line * tileE + j1];
                ca[j] = P::load(a, line, j1);
            }
        }
        for (int iz = 0; iz < zn; ++iz) {
            const double zr = zl[2 * iz], zi = zl[2 * iz + 1];
            double sr[NC], si[NC];
#pragma unroll
            for (int cc = 0; cc < NC; ++cc) sr[cc] = si[cc] = 0.0;
            if (active) {
                // the 2^d complex logs of z - e_corner, once for the cell's d! simplices
                Corner g[NV];
#pragma unroll
                for (int j = 0; j < NV; ++j) {
                    const double ur = zr - c[j];
                    g[j] = P::make({c[j], 0.5 * log(ur * ur + zi * zi), atan2(zi, ur)}, ca[j]);
                }
                if constexpr (D == 3) {
                    // the permutation (X, Y, Z) of the axes: corners 0, e_X, e_X + e_Y, (1,1,1); a loop, the corners by selects
#pragma unroll 1
                    for (int t = 0; t < 6; ++t) {
                        const int X = t >> 1, Y = (X + 1 + (t & 1)) % 3;
                        const int bb = (1 << X) | (1 << Y);
                        Corner q[4] = {g[0], green_sel(X == 0, g[1], green_sel(X == 1, g[2], g[4])),
                                       green_sel(bb == 3, g[3], green_sel(bb == 5, g[5], g[6])), g[7]};
                        P::simplex(q, zr, zi, sr, si);
                    }
                } else if constexpr (D == 2) {
#pragma unroll 1
                    for (int t = 0; t < 2; ++t) {
                        Corner q[3] = {g[0], green_sel(t == 0, g[1], g[2]), g[3]};
                        P::simplex(q, zr, zi, sr, si);
                    }
                } else {
                    Corner q[2] = {g[0], g[1]};
                    P::simplex(q, zr, zi, sr, si);
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
    const double* h = ldsg + 2 * zn;
    const size_t w = (size_t)2 * NC * zn;  // from one wave's sums to the next
    for (int t = threadIdx.x; t < 2 * NC * zn; t += 256)
        partial[(int64_t)((typename P::Col)2 * NC * z0 + t) * nrows + prow] = (h[t] + h[w + t]) + (h[2 * w + t] + h[3 * w + t]);
}

using LtmGreenFn = void (*)(abz_ctx*, dim3, size_t, const GreenWArgs&, double*, int64_t);
template <int D, class P>
void ltm_green(abz_ctx* ctx, dim3 grid, size_t lds, const GreenWArgs& a, double* partial, int64_t nrows) {
    // (the trace takes its GreenArgs part)
    launch(ctx, (ltm_green_kernel<D, P>), grid, dim3(256), (unsigned)lds, static_cast<typename P::Args>(a), partial, nrows);
}
// [d - 1][trace, NC = 1, 2, 4]
constexpr LtmGreenFn LTM_GREEN[3][4] = {
    {ltm_green<1, GreenTrace>, ltm_green<1, GreenElems<1>>, ltm_green<1, GreenElems<2>>, ltm_green<1, GreenElems<4>>},
    {ltm_green<2, GreenTrace>, ltm_green<2, GreenElems<1>>, ltm_green<2, GreenElems<2>>, ltm_green<2, GreenElems<4>>},
    {ltm_green<3, GreenTrace>, ltm_green<3, GreenElems<1>>, ltm_green<3, GreenElems<2>>, ltm_green<3, GreenElems<4>>},
};

// The scan behind launch_ltm_green (A == nullptr: the trace, one "component") and launch_ltm_green_weighted.  z_host [nz][2] with
// Im z != 0, out_host [nz][ncomp][2].  Im z < 0: the conjugate of the value at conj(z), to the bit (the elements are real).
int ltm_green_scan(abz_ctx* ctx, int n, int d, int npt, PlaneView E, const PlaneView* A, int ncomp, const double* z_host, int nz,
                   double* out_host) {
    GreenWArgs a{};  // the superset: the trace's kernel takes its GreenArgs part
    a.E = E;
    a.npt = npt;
    a.ncell = 1;
    for (int j = 0; j < d; ++j) a.ncell *= npt;
    if (A) {
        a.A = *A;
        a.acomp = (int64_t)n * A->pitch;
    }
    // of a simplex and, with elements, of its d + 1 corner weights the 1 / (m + 1)
    const double weight = 1.0 / ((double)ltm_nsimplex(d) * (double)a.ncell * (double)(A ? d + 1 : 1));
    std::vector<double> zup(2 * (size_t)nz);
    for (size_t i = 0; i < (size_t)nz; ++i) {
        zup[2 * i] = z_host[2 * i];
        zup[2 * i + 1] = std::fabs(z_host[2 * i + 1]);
    }
    // the scans' grid: one block row per band, enough blocks to fill the device several times over, few enough partial rows
    const int64_t nblocks = std::min<int64_t>(cdiv64(a.ncell, 256), std::max(64, std::min(2048, 8192 / n)));
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
    const SumOut so = sum_out_mailbox(ctx, out_host, ncols);
    double2* where = nullptr;
    if ((rc = sum_target(ctx, so, 0, (int64_t)ncols, &where))) return rc;
    // groups of 4 components, then 2, then 1 (the trace: one of 1); every group walks the grid once per chunk of z
    for (int c0 = 0; c0 < ncomp;) {
        const int nc = ncomp - c0 >= 4 ? 4 : (ncomp - c0 >= 2 ? 2 : 1);
        const int CH = green_w_chunk(nc);
        a.aplane0 = c0 * n;
        for (int s0 = 0; s0 < nz; s0 += CH) {
            const int cnt = std::min(CH, nz - s0);
            // where the cells give fewer than ~2048 blocks the values of z are dealt to blockIdx.z, at least 4 per block
            const int nsplit = (int)std::max<int64_t>(1, std::min<int64_t>(cdiv64(2048, nrows), cdiv64(cnt, 4)));
            a.z = zdev + 2 * (size_t)s0;
            a.nz = cnt;
            a.zper = (int)cdiv64(cnt, nsplit);
            const dim3 grid((unsigned)nblocks, (unsigned)n, (unsigned)cdiv64(cnt, a.zper));
            ProfScope ps(ctx, ABZ_K_LTM);
            LTM_GREEN[d - 1][A ? 1 + (nc >> 1) : 0](ctx, grid, sizeof(double) * (size_t)(2 + 8 * nc) * (size_t)a.zper, a, partial, nrows);
            ABZ_HIP(hipGetLastError());
            // column (i nc + c) 2 + t of the launch -> out[s0 + i][c0 + c][t]
            if ((rc = launch_ltm_final(ctx, partial, nrows, weight, 2 * nc * cnt, 2 * nc, 2 * ncomp,
                                       reinterpret_cast<double*>(where + ((size_t)s0 * (size_t)ncomp + (size_t)c0)))))
                return rc;
        }
        c0 += nc;
    }
    if ((rc = sum_deliver(ctx, so, where, 0, (int64_t)ncols))) return rc;
    for (size_t i = 0; i < (size_t)nz; ++i)
        if (z_host[2 * i + 1] < 0.0)
            for (size_t c = 0; c < (size_t)ncomp; ++c) out_host[2 * (i * (size_t)ncomp + c) + 1] = -out_host[2 * (i * (size_t)ncomp + c) + 1];
    return ABZ_OK;
}
}  // namespace

int launch_ltm_green(abz_ctx* ctx, int n, int d, int npt, PlaneView E, const double* z_host, int nz, double* out_host) {
    return ltm_green_scan(ctx, n, d, npt, E, nullptr, 1, z_host, nz, out_host);
}

int launch_ltm_green_weighted(abz_ctx* ctx, int n, int d, int npt, PlaneView E, PlaneView A, int ncomp, const double* z_host, int nz,
                              double* out_host) {
    return ltm_green_scan(ctx, n, d, npt, E, &A, ncomp, z_host, nz, out_host);
}

}  // namespace abz
