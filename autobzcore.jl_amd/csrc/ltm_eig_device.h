// The eigen-solve frame of the element kernels of the tetrahedron method: orbital weights and band projectors
// (kernels_ltm_orb.hip), operator expectations (kernels_ltm_expect.hip), pair elements (kernels_ltm_pairs.hip) and the density
// matrix (kernels_ltm_dens.hip).  All of them read the upper triangle of Hermitian planes (H, operators; either plane layout),
// solve per node -- 1...4 bands: one grid point per lane, herm_eig<N, true>; 5...32 bands: NP = 8 / 16 / 32 lanes per node,
// rows_eigh_columns (rows_eigvec.h) -- and differ in what they form from U.  Here is what they share: the plane index, the two
// loads, the head of a pass of the row kernels, the write-out of an LDS tile, the projector products, reads and writes of a
// register array at a uniform run-time index, and on the host the geometry of the row kernels and the dispatch over N and NP.
// gfx950 only.
#pragma once
#include <algorithm>
#include <type_traits>
#include <utility>

#include "abz_internal.h"
#include "device_math.h"
#include "rows_device.h"
#include "rows_eigvec.h"

namespace abz {

namespace {

// plane of Re X[a][b], a <= b (Im: the next one; the diagonal of the compact layout has none)
__device__ __forceinline__ int herm_plane(const PlaneView& v, int n, int a, int b) { return v.compact ? b * b + 2 * a : 2 * (a + n * b); }

// the upper triangle of X at column i of a grid line, the rest zero: what herm_eig<N, true> takes.  (The column is widened by
// the caller, here and in herm_row_load: with an int parameter the lane kernels' register counts moved by two.)
template <int N>
__device__ __forceinline__ void herm_lane_load(const PlaneView& X, int64_t line, int64_t i, CMat<N>& h) {
    const double* __restrict__ const in = X.base + line * X.tile + i;
#pragma unroll
    for (int p = 0; p < N; ++p) {
#pragma unroll
        for (int q = 0; q < N; ++q) {
            h.re[p][q] = 0.0;
            h.im[p][q] = 0.0;
            if (p <= q) {
                const int64_t pl = herm_plane(X, N, p, q);
                h.re[p][q] = in[pl * X.pitch];
                if (p < q) h.im[p][q] = in[(pl + 1) * X.pitch];
            }
        }
    }
}

// row r of Hermitian(X) at a column of a grid line: (r, j) of the upper triangle for j >= r, the conjugate of (j, r) below the
// diagonal.  Lanes r >= n read row n - 1 and keep zeros, entries j >= n are zeros; an inactive slot passes column 0 (its lanes
// must load something in bounds: they take part in the solve's exchanges)
// Called by the expectation and pair kernels, for H and for the operators, through a local closure as they called their own
// copies (called directly, ltm_pairs_rows_kernel<16> spills 624 B instead of 520).  ltm_orb_rows_kernel, ltm_proj_rows_kernel and
// ltm_dens_rows_kernel keep this text written out: a helper is simplified on its own before it is inlined, and behind the
// call, in any signature, the compiler chose other contractions in their eigen-solves -- orbital weights at NP = 16,
// projectors at NP = 32 and the density matrix at NP = 16 left the parent's bits by one unit in the last place, and the orbital
// weights stopped being the diagonal projectors (profiles/ltm_eig_frame_vs_parent.txt).  Pin the solve's contractions before
// moving those three.
template <int NP>
__device__ __forceinline__ void herm_row_load(const PlaneView& X, int n, int r, int64_t line, int64_t column, double (&hr)[NP], double (&hi)[NP]) {
    const double* __restrict__ const in = X.base + line * X.tile + column;
    const int rr = r < n ? r : n - 1;
#pragma unroll
    for (int j = 0; j < NP; ++j) {
        hr[j] = 0.0;
        hi[j] = 0.0;
        if (j < n) {  // uniform
            const int lo = rr < j ? rr : j, up = rr < j ? j : rr;
            const int64_t pl = herm_plane(X, n, lo, up);
            const double re = in[pl * X.pitch];
            const double im = in[(pl + (lo != up ? 1 : 0)) * X.pitch];
            hr[j] = r < n ? re : 0.0;
            hi[j] = (r < n && lo != up) ? (rr < j ? im : -im) : 0.0;
        }
    }
}

// A pass of a row kernel: 256 / NP consecutive nodes of one grid line, one per slot of the workgroup.
template <int NP>
struct RowsPass {
    int slot, lane;  // this thread's node slot, its lane of the wave
    double2* park;   // the slot's room in LDS: the node's reflectors, free once the back-transformation is done
    int64_t line;
    int i0, i1;    // first column of the pass, this slot's column
    int n, r;      // bands, this lane's row (through an opaque move)
    bool wave_on;  // this wave has a node in the pass (one without keeps the barriers only)
    bool act;      // this slot has a node: i1 < npt
};
template <int NP>
__device__ __forceinline__ int rows_passes_per_line(int npt) {
    return (npt + 256 / NP - 1) / (256 / NP);
}
// the head of pass `item`; called inside the loop over the passes
template <int NP>
__device__ __forceinline__ RowsPass<NP> rows_pass(double2* lds, int64_t item, int npt, int n0) {
    constexpr int SLOTS = 256 / NP;
    RowsPass<NP> ps;
    ps.slot = threadIdx.x / NP;
    ps.lane = threadIdx.x & 63;
    ps.park = lds + (size_t)ps.slot * PARK_STRIDE<NP>;
    const int ppl = rows_passes_per_line<NP>(npt);
    ps.line = item / ppl;
    ps.i0 = (int)(item - ps.line * ppl) * SLOTS;
    // (see ggr_rows_kernel: what depends on n and r alone must not be hoisted out of the loop and kept alive through it)
    ps.n = n0;
    ps.r = threadIdx.x % NP;
    asm volatile("" : "+s"(ps.n));
    asm volatile("" : "+v"(ps.r));
    ps.wave_on = ps.i0 + (int)(threadIdx.x >> 6) * (64 / NP) < npt;
    ps.i1 = ps.i0 + ps.slot;
    ps.act = ps.i1 < npt;
    return ps;
}

// The pass's columns of every plane of the element block from the LDS tile [tile row][256 / NP + 1], as contiguous row
// segments; the line's last pass takes the padding columns along, as zeros.  Plane c n + b comes from tile row row_of(c, b).
// Between two block barriers.
template <int NP, class RowOf>
__device__ __forceinline__ void rows_tile_write(const PlaneView& A, int64_t line, int i0, int npt, int n, int nplanes, const double* tile,
                                                RowOf row_of) {
    constexpr int SLOTS = 256 / NP;
    constexpr int TS = SLOTS + 1;
    const int width = (i0 + SLOTS >= npt) ? A.row - i0 : SLOTS;
    double* __restrict__ const out = A.base + line * A.tile + i0;
    for (int idx = threadIdx.x; idx < nplanes * width; idx += 256) {
        const int pl = idx / width, sl = idx - pl * width;
        const int c = pl / n, b = pl - c * n;
        out[(int64_t)pl * A.pitch + sl] = (i0 + sl < npt) ? tile[row_of(c, b) * TS + sl] : 0.0;
    }
}

// the band projector U_pb conj(U_qb) from the entries p and q of column b: the diagonal (the orbital weight), Re and Im.  One
// definition: the orbital weights, the projectors and the density matrix agree to the bit
__device__ __forceinline__ double proj_diag(double re, double im) { return fma(re, re, im * im); }
__device__ __forceinline__ double proj_re(double pr, double pi, double qr, double qi) { return fma(pr, qr, pi * qi); }
__device__ __forceinline__ double proj_im(double pr, double pi, double qr, double qi) { return fma(pi, qr, -(pr * qi)); }

// q[i] of the register array and q[k] = v, i and k uniform: select chains over values that were read first (with the element
// read inside the conditional expression the chain became a chain of addresses and one load at a run-time offset: the array
// left the registers)
template <int K, int... M>
__device__ __forceinline__ double xp_pick(const double (&q)[K], int i, std::integer_sequence<int, M...>) {
    double v = q[0];
    ((void)([&] {
         const double x = q[M + 1];
         v = (i == M + 1) ? x : v;
     }()),
     ...);
    return v;
}
template <int K>
__device__ __forceinline__ double xp_pick(const double (&q)[K], int i) {
    return xp_pick(q, i, std::make_integer_sequence<int, K - 1>());
}
template <int K, int... M>
__device__ __forceinline__ void xp_put(double (&q)[K], int k, double v, std::integer_sequence<int, M...>) {
    ((void)([&] {
         const double old = q[M];
         q[M] = (k == M) ? v : old;
     }()),
     ...);
}
template <int K>
__device__ __forceinline__ void xp_put(double (&q)[K], int k, double v) {
    xp_put(q, k, v, std::make_integer_sequence<int, K>());
}

// ---- host: geometry of the row kernels, dispatch over the compiled sizes ----------------------------------------------------
inline int rows_np(int n) { return n <= 8 ? 8 : (n <= 16 ? 16 : 32); }
// one workgroup per pass, at most `cap`
inline int64_t rows_blocks(int np, int npt, int64_t nlines, int64_t cap) {
    const int slots = 256 / np;
    return std::min<int64_t>(nlines * ((npt + slots - 1) / slots), cap);
}
// the rooms of a workgroup's 256 / np slots (PARK_STRIDE<NP> complex numbers each)
inline size_t rows_room_bytes(int np) { return sizeof(double2) * (size_t)(256 / np) * (size_t)(np * (np + 1) / 2 + 1); }
static_assert(PARK_STRIDE<8> == 8 * 9 / 2 + 1 && PARK_STRIDE<16> == 16 * 17 / 2 + 1 && PARK_STRIDE<32> == 32 * 33 / 2 + 1,
              "rows_room_bytes restates PARK_STRIDE");
// the rooms, then what the kernel keeps behind them
inline size_t rows_lds_bytes(int np, size_t tile_bytes) { return rows_room_bytes(np) + tile_bytes; }
// the tile rows_tile_write takes: NP bands of ncomp components
inline size_t rows_tile_bytes(int np, int ncomp) { return sizeof(double) * (size_t)ncomp * np * (256 / np + 1); }

// f(std::integral_constant<int, N>) for the lane kernels' N = n = 1...4, for the row kernels' NP = 8 / 16 / 32
template <class F>
int lanes_dispatch(int n, F&& f) {
    switch (n) {
        case 1: return f(std::integral_constant<int, 1>());
        case 2: return f(std::integral_constant<int, 2>());
        case 3: return f(std::integral_constant<int, 3>());
        default: return f(std::integral_constant<int, 4>());
    }
}
template <class F>
int rows_dispatch(int np, F&& f) {
    switch (np) {
        case 8: return f(std::integral_constant<int, 8>());
        case 16: return f(std::integral_constant<int, 16>());
        default: return f(std::integral_constant<int, 32>());
    }
}
// a lane kernel over the padded rows of nlines grid lines
template <class Args>
int launch_lanes(abz_ctx* ctx, void (*kernel)(Args), int64_t nlines, int row, const Args& a) {
    launch(ctx, kernel, dim3((unsigned)((nlines * row + 255) / 256)), dim3(256), 0, a);
    return ABZ_OK;
}
// a row kernel with its dynamic LDS
template <class Args>
int launch_rows(abz_ctx* ctx, void (*kernel)(Args), dim3 grid, size_t lds, const Args& a) {
    ABZ_HIP(hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    launch(ctx, kernel, grid, dim3(256), lds, a);
    return ABZ_OK;
}

}  // namespace

}  // namespace abz
