// Linear tetrahedron method (gfx950 only): DOS g(E) and state count N(E) from the cached eigenvalues of a full grid.
//
// Bloechl, Jepsen, Andersen, PRB 49, 16223 (1994), without the curvature correction.  The reference has no
// counterpart: src/dos_algorithms.jl:1-7 names "LTM" as planned.
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
//  * Shape: that of ggr_window_kernel (kernels_ggr.hip).  The energies are ascending and live in LDS; blockIdx.y is the
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
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "abz_internal.h"

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

// One tetrahedron with corner energies (a, b, c, d) in any order; i0 = first energy >= the cell's minimum.
template <bool STATES>
__device__ __forceinline__ void ltm_simplex3(double a, double b, double c, double d, const double* Esl, int nE, int i0,
                                             double* hist, double* step) {
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

template <bool STATES>
__device__ __forceinline__ void ltm_simplex2(double a, double b, double c, const double* Esl, int nE, int i0, double* hist,
                                             double* step) {
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

template <bool STATES>
__device__ __forceinline__ void ltm_simplex1(double a, double b, const double* Esl, int nE, int i0, double* hist, double* step) {
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

// Passes with at most this many of their 256 cells queued redistribute the simplices over the block; measured on the
// 150^3 grid of 3 bands: 32 energies (a fifth of the cells queued) 0.23 ms direct, 0.14 ms queued; 256 energies (most
// cells queued) 0.28 ms direct, 0.46 ms queued.
constexpr unsigned LTM_QUEUE_MAX = 128;

// partial [STATES ? 2 nE : nE][nrows]: columns 0 .. nE-1 the formula sums, nE .. 2 nE-1 the step counts
template <int D, bool STATES>
__global__ __launch_bounds__(256) void ltm_window_kernel(LtmArgs a, double* __restrict__ partial, int64_t nrows) {
    // [nE] energies | [4 waves][nE] sums | STATES: [4 waves][nE] steps | [256] queue of a pass | [2][4] per-wave counts
    extern __shared__ __attribute__((aligned(16))) double ldsl[];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nE = a.nE;
    constexpr int NH = STATES ? 8 : 4;
    constexpr int NS = D == 3 ? 6 : (D == 2 ? 2 : 1);  // simplices per cell
    const double* const Esl = ldsl;
    double* const hist = ldsl + (size_t)(1 + wave) * nE;
    double* const step = ldsl + (size_t)(5 + wave) * nE;  // STATES only
    uint32_t* const queue = reinterpret_cast<uint32_t*>(ldsl + (size_t)(1 + NH) * nE);
    uint32_t* const wcount = queue + 256;
    for (int i = threadIdx.x; i < nE; i += 256) ldsl[i] = a.Es[i];
    for (int i = threadIdx.x; i < NH * nE; i += 256) ldsl[nE + i] = 0.0;
    __syncthreads();
    const int npt = a.npt;
    const double* __restrict__ const Eb = a.E.base + (int64_t)blockIdx.y * a.E.pitch;
    const int64_t tile = a.E.tile;
    // eigenvalue at corner `bits` (bit j: +1 along variable j+1, wrapped) of cell k
    auto corner = [&](int i1, int i2, int i3, int bits) -> double {
        if ((bits & 1) && ++i1 == npt) i1 = 0;
        if (D >= 2 && (bits & 2) && ++i2 == npt) i2 = 0;
        if (D == 3 && (bits & 4) && ++i3 == npt) i3 = 0;
        return Eb[((int64_t)i3 * npt + i2) * tile + i1];
    };
    // Two passes over 256 cells at a time (the trip count is the block's, so the barriers are uniform).  Pass 1, one cell
    // per thread: the cell's window against the energy list; cells that hold an energy are queued, in thread order.  Pass 2,
    // one (queued cell, simplex) per thread: in a coarse sweep a fifth of the cells holds an energy, and a wave that walked
    // the 6 simplices of its own cells would do so for nearly every cell (some lane always has one) with most lanes idle.
    unsigned pass = 0;
    for (int64_t base = (int64_t)blockIdx.x * 256; base < a.ncell; base += (int64_t)gridDim.x * 256) {
        const int64_t k = base + threadIdx.x;
        bool active = false;
        int i0 = 0;
        double c[1 << D];
        if (k < a.ncell) {
            // k < 2^32 on every grid that fits in HBM: 32-bit division
            const int64_t line = k <= 0xffffffffll ? (int64_t)((uint32_t)k / (uint32_t)npt) : k / npt;
            const int i1 = (int)(k - line * npt);
            const int i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
            const int i2 = (int)line - i3 * npt;
#pragma unroll
            for (int j = 0; j < (1 << D); ++j) c[j] = corner(i1, i2, i3, j);
            double cmin = c[0], cmax = c[0];
#pragma unroll
            for (int j = 1; j < (1 << D); ++j) {
                cmin = fmin(cmin, c[j]);
                cmax = fmax(cmax, c[j]);
            }
            i0 = ltm_first(Esl, nE, a.inv_step, cmin);
            if (i0 < nE) {  // else every energy lies below the cell
                if (Esl[i0] < cmax) active = true;
                else if (STATES) ltm_add(step + i0, (double)NS);  // no energy inside the window: all simplices step at the same index
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
            // Most cells hold an energy (a fine sweep): every thread walks the simplices of its own cell from the corners
            // it still holds; the queue would only add its reloads.  `total` is the block's: a uniform branch.
            if (active) {
                if constexpr (D == 3) {
                    ltm_simplex3<STATES>(c[0], c[1], c[3], c[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES>(c[0], c[1], c[5], c[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES>(c[0], c[2], c[3], c[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES>(c[0], c[2], c[6], c[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES>(c[0], c[4], c[5], c[7], Esl, nE, i0, hist, step);
                    ltm_simplex3<STATES>(c[0], c[4], c[6], c[7], Esl, nE, i0, hist, step);
                } else if constexpr (D == 2) {
                    ltm_simplex2<STATES>(c[0], c[1], c[3], Esl, nE, i0, hist, step);
                    ltm_simplex2<STATES>(c[0], c[2], c[3], Esl, nE, i0, hist, step);
                } else {
                    ltm_simplex1<STATES>(c[0], c[1], Esl, nE, i0, hist, step);
                }
            }
            continue;
        }
        if (active) queue[off + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = ((uint32_t)i0 << 8) | threadIdx.x;
        __syncthreads();  // the next pass writes the queue after its own first barrier
        for (uint32_t p = threadIdx.x; p < NS * total; p += 256) {
            const uint32_t cell = p / NS, t = p - cell * NS;
            const uint32_t q = queue[cell];
            const int64_t kq = base + (q & 255u);
            const int j0 = (int)(q >> 8);
            const int64_t line = kq <= 0xffffffffll ? (int64_t)((uint32_t)kq / (uint32_t)npt) : kq / npt;
            const int i1 = (int)(kq - line * npt);
            const int i3 = D == 3 ? (int)((uint32_t)line / (uint32_t)npt) : 0;
            const int i2 = (int)line - i3 * npt;
            const double c0 = corner(i1, i2, i3, 0), c1 = corner(i1, i2, i3, (1 << D) - 1);
            if constexpr (D == 3) {
                // the permutation (A, B, C) of the axes: corners 0, e_A, e_A + e_B, (1,1,1)
                const int A = (int)(t >> 1), B = (A + 1 + (int)(t & 1)) % 3;
                const double ca = corner(i1, i2, i3, 1 << A), cb = corner(i1, i2, i3, (1 << A) | (1 << B));
                ltm_simplex3<STATES>(c0, ca, cb, c1, Esl, nE, j0, hist, step);
            } else if constexpr (D == 2) {
                ltm_simplex2<STATES>(c0, corner(i1, i2, i3, 1 << t), c1, Esl, nE, j0, hist, step);
            } else {
                ltm_simplex1<STATES>(c0, c1, Esl, nE, j0, hist, step);
            }
        }
    }
    __syncthreads();
    const int64_t prow = (int64_t)blockIdx.y * gridDim.x + blockIdx.x;
    const double* h = ldsl + nE;
    // transposed partials [column][row]: the final reduction reads the rows of one column contiguously
    for (int t = threadIdx.x; t < nE; t += 256) {
        partial[(int64_t)t * nrows + prow] = (h[t] + h[nE + t]) + (h[2 * nE + t] + h[3 * nE + t]);
        if (STATES) partial[(int64_t)(nE + t) * nrows + prow] = (h[4 * nE + t] + h[5 * nE + t]) + (h[6 * nE + t] + h[7 * nE + t]);
    }
}

// out[col] = scale * sum_rows partial[col][row], one block per column, fixed summation order (ggr_final_kernel's)
__global__ __launch_bounds__(256) void ltm_final_kernel(const double* __restrict__ partial, int64_t nrows, double scale,
                                                        double* __restrict__ out) {
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
    if (threadIdx.x == 0) out[blockIdx.x] = scale * red[0];
}

// State count of a chunk: out[i] = weight * (sums[i] + steps[0] + ... + steps[i]); col = [nE sums | nE steps], nE <= 512.
// The steps are integers, their prefix sums exact.
__global__ __launch_bounds__(256) void ltm_prefix_kernel(const double* __restrict__ col, int nE, double weight, double* __restrict__ out) {
    __shared__ double st[512];
    for (int i = threadIdx.x; i < nE; i += 256) st[i] = col[nE + i];
    __syncthreads();
    for (int i = threadIdx.x; i < nE; i += 256) {
        double run = 0.0;
        for (int j = 0; j <= i; ++j) run += st[j];
        out[i] = weight * (col[i] + run);
    }
}

}  // namespace

#define ABZ_LTM_D(ST)                                                                                         \
    switch (d) {                                                                                              \
        case 1: launch(ctx, (ltm_window_kernel<1, ST>), grid, dim3(256), lds, a, partial, nrows); break;      \
        case 2: launch(ctx, (ltm_window_kernel<2, ST>), grid, dim3(256), lds, a, partial, nrows); break;      \
        default: launch(ctx, (ltm_window_kernel<3, ST>), grid, dim3(256), lds, a, partial, nrows); break;     \
    }

int launch_ltm(abz_ctx* ctx, int n, int d, int npt, PlaneView E, const double* Es_host, int nE, bool states, double* out_host) {
    LtmArgs a;
    a.E = E;
    a.npt = npt;
    a.ncell = 1;
    for (int j = 0; j < d; ++j) a.ncell *= npt;
    const double weight = 1.0 / ((d == 3 ? 6.0 : (d == 2 ? 2.0 : 1.0)) * (double)a.ncell);
    // energies per launch: (1 + 4) x 8 KB of LDS for g, (1 + 8) x 4 KB for N (+ 1 KB of queue).  Chunks are independent: the steps of all
    // simplices below a chunk's first energy land on its index 0.
    const int CH = states ? 512 : 1024;
    const int ncol = states ? 2 : 1;
    // one block row per band; enough blocks to fill the device several times over, few enough partial rows to sum
    const int64_t nblocks = std::min<int64_t>(cdiv64(a.ncell, 256), std::max(64, std::min(2048, 8192 / n)));
    const int64_t nrows = nblocks * n;
    const int chmax = std::min(nE, CH);
    int rc = ctx->scratch[1].reserve(sizeof(double) * (size_t)(nrows * chmax * ncol));
    if (rc) return rc;
    double* partial = ctx->scratch[1].as<double>();
    EnergyList el;
    if ((rc = energies_to_device(ctx, Es_host, nE, true, 2 * (size_t)CH, el))) return rc;
    double* col = el.extra;  // states: column sums of a chunk [cnt sums | cnt steps]
    a.inv_step = el.inv_step;
    for (int s0 = 0; s0 < nE; s0 += CH) {
        const int cnt = std::min(CH, nE - s0);
        a.Es = el.dev + s0;
        a.nE = cnt;
        ProfScope ps(ctx, ABZ_K_LTM);
        const size_t lds = sizeof(double) * (states ? 9 : 5) * (size_t)cnt + sizeof(uint32_t) * (256 + 8);
        const dim3 grid((unsigned)nblocks, (unsigned)n);
        if (states) {
            ABZ_LTM_D(true);
            ABZ_HIP(hipGetLastError());
            launch(ctx, ltm_final_kernel, dim3((unsigned)(2 * cnt)), dim3(256), 0, partial, nrows, 1.0, col);
            ABZ_HIP(hipGetLastError());
            launch(ctx, ltm_prefix_kernel, dim3(1), dim3(256), 0, col, cnt, weight, el.out + s0);
        } else {
            ABZ_LTM_D(false);
            ABZ_HIP(hipGetLastError());
            launch(ctx, ltm_final_kernel, dim3((unsigned)cnt), dim3(256), 0, partial, nrows, weight, el.out + s0);
        }
        ABZ_HIP(hipGetLastError());
    }
    return energies_deliver(ctx, el, out_host);
}
#undef ABZ_LTM_D

}  // namespace abz
