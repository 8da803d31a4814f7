// Device code of the innermost evaluation, shared by the grid Fourier-eval family (kernels_eval.hip) and the kernels of
// kernels.hip that evaluate the series or address rule values themselves (reduce_kernel, eval_sum_grid_kernel,
// eig_planes_kernel, velocity_kernel, node_integrand_kernel): the series of one node, plane addressing, one unit of work of
// the grid kernels and the in-kernel contraction of a line.
#pragma once
#include "abz_internal.h"
#include "device_math.h"
#include "packed_herm.h"

#include <type_traits>

namespace abz {

// Constant-address-space view of read-only coefficient sets: a wave-uniform address in this address
// space is fetched through the scalar cache (s_load_dwordx4/x8) and reaches v_fma_f64 as an SGPR
// operand; a divergent address still becomes an ordinary global_load.  Legal because the sets are
// written by an EARLIER kernel on the same stream and never inside the kernel that reads them.
struct cplx_pod {
    double x, y;
};
typedef const cplx_pod __attribute__((address_space(4))) * cptr_t;
__device__ __forceinline__ cptr_t as_const(const double2* p) {
    return (cptr_t)(unsigned long long)p;
}

// H = sum_m c1[m] * (w z^m)  (optionally times i 2 pi f_m).
template <int N>
__device__ __forceinline__ void series_lane(cptr_t c1, int M, int first, double zr,
                                            double zi, double wr, double wi, bool deriv, CMat<N>& H) {
#pragma unroll
    for (int a = 0; a < N; ++a) {
#pragma unroll
        for (int b = 0; b < N; ++b) {
            H.re[a][b] = 0.0;
            H.im[a][b] = 0.0;
        }
    }
    double pr = wr, pi = wi;
    for (int m = 0; m < M; ++m) {
        double qr = pr, qi = pi;
        if (deriv) {
            const double f = 6.283185307179586476925286766559 * (double)(first + m);
            qr = -f * pi;
            qi = f * pr;
        }
        cptr_t cm = c1 + (int64_t)m * (N * N);
#pragma unroll
        for (int b = 0; b < N; ++b) {
#pragma unroll
            for (int a = 0; a < N; ++a) {
                const double cx = cm[a + N * b].x, cy = cm[a + N * b].y;  // column-major block
                H.re[a][b] = fma(cx, qr, H.re[a][b]);
                H.re[a][b] = fma(-cy, qi, H.re[a][b]);
                H.im[a][b] = fma(cx, qi, H.im[a][b]);
                H.im[a][b] = fma(cy, qr, H.im[a][b]);
            }
        }
        const double nr = pr * zr - pi * zi;
        const double ni = pr * zi + pi * zr;
        pr = nr;
        pi = ni;
    }
}

// offset of (node k, plane 0) in a tiled planar view
__device__ __forceinline__ int64_t view_off(const PlaneView& v, int64_t k) {
    const int64_t line = k / v.line_len;
    return line * v.tile + (k - line * v.line_len);
}

// Plane of Re H[a][b], a <= b, in a view (Im is the next plane).  Full layout, the reference's SMatrix order:
// 2 (a + N b).  Hermitian-compact layout (PlaneView::compact, ABZ_WANT_H_COMPACT in abzhip.h): the upper triangle column
// by column, b^2 + 2 a; the real diagonal entry H[b][b] is the single plane b^2 + 2 b.
template <int N>
__device__ __forceinline__ int hplane(const PlaneView& v, int a, int b) {
    return v.compact ? b * b + 2 * a : 2 * (a + N * b);
}

template <int N>
__device__ __forceinline__ void store_planes(const CMat<N>& H, const PlaneView& v, int64_t off) {
    double* __restrict__ out = v.base + off;
    if (v.compact) {
#pragma unroll
        for (int b = 0; b < N; ++b) {
#pragma unroll
            for (int a = 0; a <= b; ++a) {
                out[(int64_t)(b * b + 2 * a) * v.pitch] = H.re[a][b];
                if (a < b) out[(int64_t)(b * b + 2 * a + 1) * v.pitch] = H.im[a][b];
            }
        }
        return;
    }
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int a = 0; a < N; ++a) {
            out[(int64_t)(2 * (a + N * b)) * v.pitch] = H.re[a][b];
            out[(int64_t)(2 * (a + N * b) + 1) * v.pitch] = H.im[a][b];
        }
    }
}

// Hermitian values: the upper triangle's planes only (n^2 loads instead of 2 n^2), the rest mirrored in registers
template <int N>
__device__ __forceinline__ void load_planes_herm(CMat<N>& H, const PlaneView& v, int64_t off) {
    const double* __restrict__ in = v.base + off;
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int a = 0; a <= b; ++a) {
            const int pl = hplane<N>(v, a, b);
            H.re[a][b] = in[(int64_t)pl * v.pitch];
            H.im[a][b] = (a == b) ? 0.0 : in[(int64_t)(pl + 1) * v.pitch];
        }
    }
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int a = b + 1; a < N; ++a) {
            H.re[a][b] = H.re[b][a];
            H.im[a][b] = -H.im[b][a];
        }
    }
}

template <int N>
__device__ __forceinline__ void load_planes(CMat<N>& H, const PlaneView& v, int64_t off) {
    if (v.compact) {  // only the upper triangle exists
        load_planes_herm<N>(H, v, off);
        return;
    }
    const double* __restrict__ in = v.base + off;
#pragma unroll
    for (int b = 0; b < N; ++b) {
#pragma unroll
        for (int a = 0; a < N; ++a) {
            H.re[a][b] = in[(int64_t)(2 * (a + N * b)) * v.pitch];
            H.im[a][b] = in[(int64_t)(2 * (a + N * b) + 1) * v.pitch];
        }
    }
}

struct EvalArgs {
    const double2* src;
    const double2* tab;
    const int64_t* parents;
    const int32_t* gi;
    const double* x;
    PlaneView H, E, U;
    int64_t nlines, nk;
    int64_t line0;  // store-free sums on a slab: global index of line 0 (for node coordinates)
    int M, first, npt, deriv, herm;
    int nt;  // non-temporal stores (rule values larger than the Infinity Cache)
    int pk;    // the level-1 sets are PACKED Hermitian sets (packed_herm.h): Pk<N>::size((M - 1) / 2) numbers per line
    double inv_period;
    // fused last contraction (the fused mappings of eval_grid_kernel): level-2 sets [nlines / npt][M2][numbers per line], the
    // phase table [npt][M2] of variable 2, blocks per outermost index
    const double2* src2 = nullptr;
    const double2* phs2 = nullptr;
    int M2 = 0, bpk = 0;
    // nlines == npt^2, real Hermitian series: the lines of planes k3 <= npt / 2 are evaluated, the rest stored as their mirror
    // images (eval_unit_store)
    int mirror = 0;
};

// planes of one node at column i1 of tile `line`; with a wave-uniform line every plane row is a scalar
// base and the lane offset i1 is the same 32-bit register for all of them.  NT: non-temporal stores
// (streaming: the values are not re-read by this kernel and a large rule does not fit the caches anyway).
template <bool NT>
__device__ __forceinline__ void store_f64(double* p, double v) {
    if constexpr (NT)
        __builtin_nontemporal_store(v, p);
    else
        *p = v;
}
// CONJ: the conjugate is stored (the imaginary planes with their sign flipped; the diagonal's stay as they are, +0.0 in
// Hermitian instances either way)
template <int N, bool NT = false, bool HC = false, bool CONJ = false>
__device__ __forceinline__ void store_planes_at(const CMat<N>& H, const PlaneView& v, int64_t line, int i1) {
    double* __restrict__ row = v.base + line * v.tile;
    const unsigned u = (unsigned)i1;
    if constexpr (HC) {  // Hermitian-compact planes: the upper triangle
#pragma unroll
        for (int b = 0; b < N; ++b) {
#pragma unroll
            for (int a = 0; a <= b; ++a) {
                store_f64<NT>((row + (int64_t)(b * b + 2 * a) * v.pitch) + u, H.re[a][b]);
                if (a < b) store_f64<NT>((row + (int64_t)(b * b + 2 * a + 1) * v.pitch) + u, CONJ ? -H.im[a][b] : H.im[a][b]);
            }
        }
    } else {
#pragma unroll
        for (int b = 0; b < N; ++b) {
#pragma unroll
            for (int a = 0; a < N; ++a) {
                store_f64<NT>((row + (int64_t)(2 * (a + N * b)) * v.pitch) + u, H.re[a][b]);
                store_f64<NT>((row + (int64_t)(2 * (a + N * b) + 1) * v.pitch) + u, (CONJ && a != b) ? -H.im[a][b] : H.im[a][b]);
            }
        }
    }
}

template <int N, bool VEC = true>
__device__ __forceinline__ void eval_epilogue(const EvalArgs& a, CMat<N>& H, int64_t line, int i1) {
    if (a.H.base) {
        if (a.H.compact)
            store_planes_at<N, false, true>(H, a.H, line, i1);
        else
            store_planes_at<N>(H, a.H, line, i1);
    }
    if (a.E.base || (VEC && a.U.base)) {
        double e[N];
        CMat<N> V;
        if (VEC && a.U.base) {
            herm_eig<N, true>(H, e, V);
            store_planes_at<N>(V, a.U, line, i1);
        } else {
            herm_eig_values<N>(H, e);
        }
        if (a.E.base) {
            double* __restrict__ row = a.E.base + line * a.E.tile;
            const unsigned u = (unsigned)i1;
#pragma unroll
            for (int b = 0; b < N; ++b) (row + (int64_t)b * a.E.pitch)[u] = e[b];
        }
    }
}

// One wavefront per line (i2,i3); each lane owns KPL nodes i1 = i0 + lane + 64 j of that line.
// The line's coefficients c1[M][N*N] are staged in a wave-private LDS buffer (double-buffered: the
// next line's set is fetched into registers while the current one is consumed), read back with
// broadcast ds_read_b128 and reused for the KPL nodes of every lane; phases w z^m by recurrence.
// No block-level barrier: a wave only ever reads the LDS bytes it wrote itself.
// (EVAL_MAX_MNN complex coefficients per line at most, eval_route.h)

// Phase recurrence of the grid kernels, p <- p z.  The roundings are spelled out: written as p.x z.x - p.y z.y and
// p.x z.y + p.y z.x, the compiler chose which product to fuse per instance (one column per lane: fma(p.y, z.x, p.x z.y);
// three: fma(p.x, z.y, p.y z.x)), so two work mappings of one grid agreed only by chance.  This is the form of the
// three-column instances (the 150^3 grid), now the same in every instance.
__device__ __forceinline__ void phase_step(double& pr, double& pi, double zr, double zi) {
    const double nr = fma(pr, zr, -(pi * zi));
    const double ni = fma(pr, zi, pi * zr);
    pr = nr;
    pi = ni;
}

// One unit of work of the grid kernels: pass `pass` (64 KPL nodes starting at i0) of line `line`, from the
// line's coefficients c1 (LDS).  `mid` runs between the m-loop and the stores: the place where the next
// unit's coefficients are handed to the other LDS buffer.
// LW = 32 (pair mapping of the fused instance): a unit is a pass of TWO lines, one per half-wave; `lane` is then the
// lane's index within its half, c1 its half's set, and a lane owns the columns i0 + lane + 32 j.  Per node the
// arithmetic is the same either way.
template <int N, int KPL, bool HERM, class MID, bool PK = false, int LW = 64>
__device__ __forceinline__ void eval_unit_core(const EvalArgs& a, const double2* __restrict__ c1, const double2* tab_l, int fm,
                                               const int (&iz0)[KPL], const int (&iw0)[KPL], int npass, int i0, int lane,
                                               MID&& mid, CMat<N> (&H)[KPL]) {
    if constexpr (PK) {
        // packed Hermitian set (packed_herm.h): +f and -f in one FMA group, phases z^f from z alone -- half the Fourier
        // work of the loop over 2 F + 1 terms below
        static_assert(HERM, "packed sets exist for Hermitian series only");
        const int F = (a.M - 1) / 2;
        double zr[KPL], zi[KPL], pr[KPL], pi[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            int ic = iz0[j];
            if (npass > 1) {
                const int i1 = i0 + lane + LW * j;
                ic = i1 < a.npt ? i1 : 0;
            }
            const double2 z = tab_l[ic];
            zr[j] = z.x;
            zi[j] = z.y;
            pr[j] = 1.0;
            pi[j] = 0.0;
        }
#pragma unroll
        for (int bb = 0; bb < N; ++bb) {
#pragma unroll
            for (int aa = 0; aa <= bb; ++aa) {
                const double2 c = c1[Pk<N>::tri(aa, bb)];
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    H[j].re[aa][bb] = c.x;
                    H[j].im[aa][bb] = (aa == bb) ? 0.0 : c.y;
                }
            }
        }
        for (int f = 1; f <= F; ++f) {
#pragma unroll
            for (int j = 0; j < KPL; ++j) {
                phase_step(pr[j], pi[j], zr[j], zi[j]);
            }
            const double2* __restrict__ cf = c1 + Pk<N>::blk(1) + (f - 1) * (N * N);
#pragma unroll
            for (int aa = 0; aa < N; ++aa) {
                const double2 dd = cf[aa];
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    H[j].re[aa][aa] = fma(dd.x, pr[j], H[j].re[aa][aa]);
                    H[j].re[aa][aa] = fma(-dd.y, pi[j], H[j].re[aa][aa]);
                }
            }
#pragma unroll
            for (int bb = 1; bb < N; ++bb) {
#pragma unroll
                for (int aa = 0; aa < bb; ++aa) {
                    const double2 sv = cf[N + 2 * Pk<N>::pair(aa, bb)];
                    const double2 tv = cf[N + 2 * Pk<N>::pair(aa, bb) + 1];
#pragma unroll
                    for (int j = 0; j < KPL; ++j) {
                        H[j].re[aa][bb] = fma(sv.x, pr[j], H[j].re[aa][bb]);
                        H[j].re[aa][bb] = fma(-sv.y, pi[j], H[j].re[aa][bb]);
                        H[j].im[aa][bb] = fma(tv.x, pi[j], H[j].im[aa][bb]);
                        H[j].im[aa][bb] = fma(tv.y, pr[j], H[j].im[aa][bb]);
                    }
                }
            }
        }
        mid();
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
#pragma unroll
            for (int bb = 0; bb < N; ++bb) {
#pragma unroll
                for (int aa = bb + 1; aa < N; ++aa) {
                    H[j].re[aa][bb] = H[j].re[bb][aa];
                    H[j].im[aa][bb] = -H[j].im[bb][aa];
                }
            }
        }
        return;
    }
    double zr[KPL], zi[KPL], pr[KPL], pi[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        int ic = iz0[j], iw = iw0[j];
        if (npass > 1) {
            const int i1 = i0 + lane + LW * j;
            ic = i1 < a.npt ? i1 : 0;
            iw = (int)(((unsigned)fm * (unsigned)ic) % (unsigned)a.npt);
        }
        const double2 z = tab_l[ic];
        const double2 w = tab_l[iw];
        zr[j] = z.x;
        zi[j] = z.y;
        pr[j] = w.x;
        pi[j] = w.y;
#pragma unroll
        for (int aa = 0; aa < N; ++aa) {
#pragma unroll
            for (int bb = 0; bb < N; ++bb) {
                H[j].re[aa][bb] = 0.0;
                H[j].im[aa][bb] = 0.0;
            }
        }
    }
    for (int m = 0; m < a.M; ++m) {
        const double2* __restrict__ cm = c1 + m * (N * N);
#pragma unroll
        for (int bb = 0; bb < N; ++bb) {
#pragma unroll
            for (int aa = 0; aa < N; ++aa) {
                if (HERM && aa > bb) continue;  // upper triangle only; mirrored below
                const double2 c = cm[aa + N * bb];
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    H[j].re[aa][bb] = fma(c.x, pr[j], H[j].re[aa][bb]);
                    H[j].re[aa][bb] = fma(-c.y, pi[j], H[j].re[aa][bb]);
                    if (!(HERM && aa == bb)) {
                        H[j].im[aa][bb] = fma(c.x, pi[j], H[j].im[aa][bb]);
                        H[j].im[aa][bb] = fma(c.y, pr[j], H[j].im[aa][bb]);
                    }
                }
            }
        }
#pragma unroll
        for (int j = 0; j < KPL; ++j) phase_step(pr[j], pi[j], zr[j], zi[j]);
    }
    mid();
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        if constexpr (HERM) {
#pragma unroll
            for (int bb = 0; bb < N; ++bb) {
#pragma unroll
                for (int aa = bb + 1; aa < N; ++aa) {
                    H[j].re[aa][bb] = H[j].re[bb][aa];
                    H[j].im[aa][bb] = -H[j].im[bb][aa];
                }
            }
        }
    }
}

// Where a unit's values go a second time when the rule is built from the planes k3 <= npt / 2 alone (EvalArgs::mirror): the
// row of -k.  `line` is a line of the mirrored plane and t0 / t1 the offset from it in tiles for the lanes of the first and
// of the second half-wave (the pair mapping: line = first line of the mirrored plane, t0 / t1 = the mirrored k2 of the half's
// line; the two are not neighbours at k2 = 0).  All three are scalars.
// line < 0: nothing is mirrored (the unit's plane is its own mirror image, or the launch evaluates every plane).
struct MirrorTo {
    int64_t line = -1;
    int t0 = 0, t1 = 0;
};

// The store epilogue of a unit: values of its 64 KPL nodes into the tiled-planar rule arrays.
// Pair mapping (LW = 32): `line` is the pair's first line and the second half-wave adds one tile to its lane offset
// (off_h, off_e: 0 or the tile of the H and of the eigenvalue planes), so every plane row keeps its scalar base; a
// half without a line of its own (odd npt) has `on` false and stores nothing.
// Mirror (mt.line >= 0): H(-k) = conj H(k) of a real Hermitian series, from the same registers -- column i1 of the row goes
// to column (npt - i1) % npt of the mirrored row, padding columns to themselves, with the sign of the off-diagonal imaginary
// planes flipped and the same eigenvalues.  Every column of the mirrored tile is written exactly once, like the unit's own.
// A half-wave's mirrored run is contiguous but descends with the lane and starts off a 128-B line ((npt - 32 j - 31) 8 B:
// 56 B off at 150 points), so it leaves lines partial until the next round or, across a pass seam, the next pass fills them.
// These stores are therefore always temporal, so that L2 merges the parts before the line goes out: with the unit's own
// non-temporal policy the 150^3 launch took 141 us instead of 62 (every line written to memory twice, in parts).
template <int N, int KPL, bool VEC, int LW = 64>
__device__ __forceinline__ void eval_unit_store(const EvalArgs& a, CMat<N> (&H)[KPL], int i0, int lane, int64_t line, int off_h = 0,
                                                int off_e = 0, bool on = true, const MirrorTo mt = MirrorTo()) {
    if constexpr (VEC) {
        static_assert(LW == 64, "the pair mapping stores values and eigenvalues only");
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int i1 = i0 + lane + 64 * j;
            const int pitch = a.H.base ? a.H.row : a.E.row;
            if (i1 < pitch) eval_epilogue<N, VEC>(a, H[j], line, i1);
        }
    }
    if constexpr (!VEC) {
        // columns npt..pitch-1 are padding: written (finite filler) so every 128-B line of the
        // tile leaves the CU whole; never read back (leaving them unwritten measured 17 % slower: partial lines).
        // Order: ALL H(k) stores of the unit first, then the eigensolves (they overlap the drain of those
        // stores), then the eigenvalue stores.  With non-temporal stores on rules larger than the Infinity
        // Cache this is worth 19 % at 150^3 (neither change alone is: the interleaved order leaves the
        // store queue empty during every eigensolve, and temporal stores make the 605 MB fight for L2/MALL).
        const int pitch = a.H.base ? a.H.row : a.E.row;
        const bool mir = mt.line >= 0;  // wave-uniform
        // the lane's offset in the mirrored row for its column j, formed where it is used from a thread index the compiler
        // cannot see through: hoisted out of the work loop (one register per column and pass) these offsets were spilled to
        // scratch at three waves per SIMD (the benchmark's instance, 3 bands, packed, pairs, passes of 3 and 2 rounds: 168 VGPRs and
        // 12 B of scratch per lane, reloaded in the work loop; formed here: 168 VGPRs, no scratch, three waves per SIMD).
        // This relies on what every caller passes: lane == threadIdx.x & (LW - 1), and with LW == 32 bit 5 of threadIdx.x
        // is the lane's half (eval_grid_kernel: lane = threadIdx.x & 63, col = lane & 31, half = lane >> 5).
        auto moffset = [&](int j, int64_t tile) {
            int tx = threadIdx.x;
            asm volatile("" : "+v"(tx));
            const int i1 = i0 + (tx & (LW - 1)) + LW * j;
            const int mc = (i1 == 0 || i1 >= a.npt) ? i1 : a.npt - i1;
            return mc + (LW == 32 && (tx & 32) ? mt.t1 : mt.t0) * (int)tile;
        };
        auto epilogue = [&](auto nt, auto hc) {
            constexpr bool NT = decltype(nt)::value;
            constexpr bool HC = decltype(hc)::value;
            if (a.H.base) {
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    const int i1 = i0 + lane + LW * j;
                    if (i1 < pitch && on) store_planes_at<N, NT, HC>(H[j], a.H, line, i1 + off_h);
                }
                if (mir) {
#pragma unroll
                    for (int j = 0; j < KPL; ++j) {
                        const int i1 = i0 + lane + LW * j;
                        if (i1 < pitch && on) store_planes_at<N, false, HC, true>(H[j], a.H, mt.line, moffset(j, a.H.tile));
                    }
                }
            }
            if (a.E.base) {
#pragma unroll
                for (int j = 0; j < KPL; ++j) {
                    const int i1 = i0 + lane + LW * j;
                    if (i1 < pitch && on) {
                        double e[N];
                        herm_eig_values<N>(H[j], e);
                        double* __restrict__ row = a.E.base + line * a.E.tile;
                        const unsigned u = (unsigned)(i1 + off_e);
#pragma unroll
                        for (int b = 0; b < N; ++b) store_f64<NT>((row + (int64_t)b * a.E.pitch) + u, e[b]);
                        if (mir) {
                            double* __restrict__ mrow = a.E.base + mt.line * a.E.tile;
                            const unsigned mu = (unsigned)moffset(j, a.E.tile);
#pragma unroll
                            for (int b = 0; b < N; ++b) store_f64<false>((mrow + (int64_t)b * a.E.pitch) + mu, e[b]);
                        }
                    }
                }
            }
        };
        if (a.H.compact) {
            if (a.nt)
                epilogue(std::true_type{}, std::true_type{});
            else
                epilogue(std::false_type{}, std::true_type{});
        } else if (a.nt)
            epilogue(std::true_type{}, std::false_type{});
        else
            epilogue(std::false_type{}, std::false_type{});
    }
}

template <int N, int KPL, bool HERM, bool VEC, class MID, bool PK = false, int LW = 64>
__device__ __forceinline__ void eval_unit(const EvalArgs& a, const double2* __restrict__ c1, const double2* tab_l, int fm,
                                          const int (&iz0)[KPL], const int (&iw0)[KPL], int npass, int i0, int lane,
                                          int64_t line, MID&& mid, int off_h = 0, int off_e = 0, bool on = true,
                                          const MirrorTo mt = MirrorTo()) {
    CMat<N> H[KPL];
    eval_unit_core<N, KPL, HERM, MID&, PK, LW>(a, c1, tab_l, fm, iz0, iw0, npass, i0, lane, mid, H);
    eval_unit_store<N, KPL, VEC, LW>(a, H, i0, lane, line, off_h, off_e, on, mt);
}

__device__ __forceinline__ void wave_lds_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// Fused last contraction (the fused mappings of eval_grid_kernel): one line's level-1 set from the level-2 set s2[M2][MNN] of its
// outermost index (LDS) and the phases of its k2 (wave-uniform address: scalar loads), lane = column, with the very fma
// sequence of contract_grid_s_kernel / contract_chain_kernel for m ascending -- the sums are theirs bit for bit.
// The phases are fetched as a fixed group of ABZ_CONTRACT_GRID_MAXM, whatever M2 is (straight-line scalar loads that can
// be issued ahead of the block's barrier): the table is readable that far past the start of any row (EvalSpec::phs2).
struct LinePhases {
    double x[ABZ_CONTRACT_GRID_MAXM], y[ABZ_CONTRACT_GRID_MAXM];
};
__device__ __forceinline__ void load_line_phases(cptr_t p, LinePhases& ph) {
#pragma unroll
    for (int m = 0; m < ABZ_CONTRACT_GRID_MAXM; ++m) {
        ph.x[m] = p[m].x;
        ph.y[m] = p[m].y;
    }
}

template <int M2>
__device__ __forceinline__ void contract_line(const double2* s2, const LinePhases& ph, double2* dst, int MNN, int lane) {
    for (int l = lane; l < MNN; l += 64) {
        double ar = 0.0, ai = 0.0;
#pragma unroll
        for (int m = 0; m < M2; ++m) {
            const double2 c = s2[m * MNN + l];
            ar = fma(c.x, ph.x[m], ar);
            ar = fma(-c.y, ph.y[m], ar);
            ai = fma(c.x, ph.y[m], ai);
            ai = fma(c.y, ph.x[m], ai);
        }
        dst[l] = make_double2(ar, ai);
    }
}

__device__ __forceinline__ void contract_line_m(int M2, const double2* s2, const LinePhases& ph, double2* dst, int MNN, int lane) {
#define CL(MM) case MM: contract_line<MM>(s2, ph, dst, MNN, lane); break;
    switch (M2) {  // exact coefficient count: straight-line code
        CL(1) CL(2) CL(3) CL(4) CL(5) CL(6) CL(7) CL(8) CL(9) CL(10) CL(11) CL(12) CL(13) CL(14) CL(15) CL(16)
        default: break;  // eval_route admits 1 ... ABZ_CONTRACT_GRID_MAXM only
    }
#undef CL
}

}  // namespace abz
