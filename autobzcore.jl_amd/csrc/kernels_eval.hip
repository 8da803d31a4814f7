// The grid Fourier-eval family, written for gfx950 (MI355X, wave64) only.
//
//   eval_grid_kernel         innermost 1-D series on a full PTR grid: one wavefront per pass of a line (i2,i3),
//                            KPL nodes per lane, the line's coefficients in a wave-private double-buffered LDS
//                            slot, one load group and one wait per unit of work (in-order vmcnt), fused
//                            Hermitian eigensolve, tiled-planar stores (H first, non-temporal on large rules)
//                            = workspace_evaluate! in fourier_ptr!  (ref src/fourier.jl:132-147)
//   eval_grid_kernel_scalar  the same for coefficient sets too large for LDS
//   eval_node_kernel         the series at explicit nodes (symmetric rules, abz_eval_nodes)
//
// Which instance of eval_grid_kernel runs, on what launch grid and with how much LDS is decided by eval_route
// (eval_route.h, host-only); launch_eval reads the route and launches.  The device code shared with kernels.hip is in
// eval_device.h.
#include "abz_internal.h"
#include "eval_device.h"

#include <type_traits>

namespace abz {

// One instance of eval_grid_kernel, every argument named.
//   N, HERM, VEC, PK  bands; Hermitian series (upper triangle only); eigenvectors stored; packed Hermitian sets
//   KPL, KT           nodes per lane (pair mappings: rounds of 32 columns) of a pass, and of the last pass
//   MAP               the work mapping (EvalMapping, eval_route.h):
//     streamed        the level-1 sets come from memory, prefetched into registers a unit ahead.
//     fused_lines     the level-1 sets never exist in memory.  A block owns one outermost index k3 and the lines
//                     k2 = 4 seg + wave, stepping by 4 bpk, of that index; it stages the level-2 set of k3 next to the phase
//                     table (one round trip) and every wave contracts its next line into its other LDS buffer where the
//                     streamed mapping hands over prefetched registers: the work loop holds no vector load at all.
//     fused_pairs     one grid line per half-wave.  A wave's unit is the pair of lines (k2, k2 + 1), k2 = 2 (4 seg + wave)
//                     stepping by 8 bpk: lanes 0-31 own line k2, lanes 32-63 line k2 + 1, a lane the columns (lane & 31) + 32 j.
//                     Five rounds cover a 160-double row exactly where the 64-lane mapping issues 3 x 64 = 192 slots per line.
//                     The rounds of a pair, ceil(npt / 32), are run as passes of KPL with a last pass of KT <= KPL (150 points:
//                     3 + 2; five rounds in one pass spill at three waves per SIMD), so no round is idle.  Both lines' level-1
//                     sets lie side by side in the wave's LDS room, [buffer][half][MNN]; k3, the pair and the pass stay
//                     scalars, only the half is per lane (the set's address and one tile added to the store offset).  The last
//                     pair of an odd npt has one line: its second half evaluates line npt - 1 again and stores nothing.
//     fused_passwave  (Hermitian series) one pass of one pair per wave.  The unit u = 4 seg + wave is pass u % npass of pair
//                     u / npass, with npass = 2 or 4 (eval_route), so the passes of a pair sit in one block: the two parts of a
//                     mirrored 128-B line at a pass seam meet in one L2.  The wave contracts both lines of its pair as above --
//                     each of a pair's npass waves does, the sums are the same -- runs its pass, KPL rounds or the last pass's
//                     KT, stores and ends: no work loop, one LDS buffer per wave and nothing contracted between the m-loop and
//                     the stores.  A template parameter as MIR is: other instances hold none of its code.
//   MIR               the instance of a mirrored launch (EvalArgs::mirror, Hermitian series only).  A template parameter, so the
//                     instances of every other launch hold none of its code: with a run-time flag alone the benchmark's
//                     instance measured 5 % slower with the mirror switched off.
template <int N_, int KPL_, int KT_, bool HERM_, bool VEC_, bool PK_, EvalMapping MAP_, bool MIR_>
struct EvalCfg {
    static constexpr int N = N_, KPL = KPL_, KT = KT_;
    static constexpr bool HERM = HERM_, VEC = VEC_, PK = PK_, MIR = MIR_;
    static constexpr EvalMapping MAP = MAP_;
    static constexpr bool FUSE = MAP != EvalMapping::streamed;
    static constexpr bool PW = MAP == EvalMapping::fused_passwave;
    static constexpr bool PAIR = PW || MAP == EvalMapping::fused_pairs;
    static constexpr int OCC = eval_occupancy(N, HERM);
    static constexpr int LPU = PAIR ? 2 : 1;  // lines per unit of work
    static constexpr int LW = 64 / LPU;       // lanes per line
    static constexpr int NBUF = PW ? 1 : 2;   // LDS buffers per wave
    static_assert(MAP == EvalMapping::streamed || MAP == EvalMapping::fused_lines || PAIR, "a mapping of eval_grid_kernel");
    static_assert(!MIR || (HERM && !VEC), "MIR: values and eigenvalues of a Hermitian series");
    static_assert(!PK || HERM, "PK: packed sets exist for Hermitian series only");
    static_assert(!FUSE || !VEC, "the fused mappings store values and eigenvalues only");
    static_assert(KT >= 1 && KT <= KPL && (PAIR || KT == KPL), "KT < KPL: a shorter last pass exists in the pair mappings only");
    static_assert(!PW || HERM, "fused_passwave exists for Hermitian series only");
};

template <class C>
__global__ __launch_bounds__(256, C::OCC) void eval_grid_kernel(EvalArgs a) {
    constexpr int N = C::N, KPL = C::KPL, KT = C::KT, LPU = C::LPU, LW = C::LW, NBUF = C::NBUF;
    constexpr bool HERM = C::HERM, VEC = C::VEC, PK = C::PK, FUSE = C::FUSE, PAIR = C::PAIR, MIR = C::MIR, PW = C::PW;
    extern __shared__ double2 lds_c[];  // [4 waves][NBUF buffers][LPU][MNN], phase table [npt], fused: level-2 set [M2][MNN]
    // the wave index is made an SGPR value: every per-line quantity (tile base, coefficient row) is
    // then scalar arithmetic
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int MNN = PK ? Pk<N>::size((a.M - 1) / 2) : a.M * N * N;  // numbers per line
    // derivative series: coefficient m is scaled by 2 pi i (first + m) once, on its way into LDS
    auto stage = [&](double2 c, int idx) -> double2 {
        if (!a.deriv) return c;
        const double f = 6.283185307179586476925286766559 * (double)(a.first + idx / (N * N));
        return make_double2(-f * c.y, f * c.x);
    };
    double2* const mybuf = lds_c + (size_t)wave * NBUF * LPU * MNN;
    int fm = a.first % a.npt;
    if (fm < 0) fm += a.npt;
    // Every global load issued inside the work loop shares the in-order vmcnt with the stores, and a
    // wait on any of them is a wait on every older store of the wave.  So the loop body is straight
    // line code with exactly one group of loads (the next unit's coefficients) and one wait, placed
    // right after the m-loop when the previous unit's stores are a whole m-loop old; phase seeds
    // come from an LDS copy of the table.  A unit of work is one pass (64 KPL nodes) of one line.
    const int npass = (a.npt + LW * KPL - 1) / (LW * KPL);
    double2* const tab_l = lds_c + (size_t)4 * NBUF * LPU * MNN;  // LDS copy of the phase table, shared by the block
    if constexpr (FUSE) {
        const int k3 = blockIdx.y, seg = blockIdx.x;  // grid (bpk, outermost indices): both scalars
        // mirror: the grid's rows are the planes k3 <= npt / 2; the plane of -k3, or -1 where k3 is its own (0 and npt / 2)
        const int mk3 = (MIR && k3 != 0 && 2 * k3 != a.npt) ? a.npt - k3 : -1;
        const int L2 = a.M2 * MNN;
        const double2* __restrict__ src2 = a.src2 + (int64_t)k3 * L2;
        double2* const s2 = tab_l + a.npt;
        // the phases of the wave's first line: in flight across the copy and the barrier (a wave beyond the last line
        // reads row 0)
        const int kstride = 4 * a.bpk;
        int k2 = LPU * (4 * seg + wave);
        int pw_pass = 0;  // fused_passwave: the wave's pass of its pair; npass is 2 or 4
        if constexpr (PW) {
            const int u = 4 * seg + wave;
            pw_pass = u & (npass - 1);
            k2 = 2 * (u >> (npass == 4 ? 2 : 1));
        }
        LinePhases ph;
        load_line_phases(as_const(a.phs2 + (int64_t)(k2 < a.npt ? k2 : 0) * a.M2), ph);
        // phase table and level-2 set in one round trip: the loads are unconditional, from clamped 32-bit indices off
        // scalar bases, and the asm keeps the stores' bounds checks from being hoisted above them
        {
            const int it = threadIdx.x;
            double2 vt = a.tab[min(it, a.npt - 1)];
            double2 v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = src2[min(it + 256 * j, L2 - 1)];
            asm volatile("" : "+v"(vt.x), "+v"(vt.y));
#pragma unroll
            for (int j = 0; j < 4; ++j) asm volatile("" : "+v"(v[j].x), "+v"(v[j].y));
            if (it < a.npt) tab_l[it] = vt;
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (it + 256 * j < L2) s2[it + 256 * j] = v[j];
            for (int i = it + 256; i < a.npt; i += 256) tab_l[i] = a.tab[i];       // (more than 256 points)
            for (int i = it + 4 * 256; i < L2; i += 256) s2[i] = src2[i];          // (more than 1024 numbers)
        }
        __syncthreads();
        if (k2 >= a.npt) return;
        contract_line_m(a.M2, s2, ph, mybuf, MNN, lane);
        if constexpr (PAIR) {
            const int half = lane >> 5, col = lane & 31;
            // both lines of a pair, one after the other, lane = column as above; line k2 + 1 clamped to the last line
            load_line_phases(as_const(a.phs2 + (int64_t)min(k2 + 1, a.npt - 1) * a.M2), ph);
            contract_line_m(a.M2, s2, ph, mybuf + MNN, MNN, lane);
            if constexpr (PW) {
                // the wave's one unit; its seeds come from the column (two passes at least: the seeds of pass 0 are not read)
                const int seeds[KPL] = {}, seeds_t[KT] = {};
                const int64_t line = (int64_t)k3 * a.npt + k2;
                MirrorTo mt;
                if (mk3 >= 0) {
                    mt.line = (int64_t)mk3 * a.npt;
                    mt.t0 = k2 ? a.npt - k2 : 0;
                    mt.t1 = k2 + 1 < a.npt ? a.npt - k2 - 1 : 0;  // (a half without a line: nothing is stored)
                }
                auto no_mid = []() {};
                wave_lds_sync();
                if (KT == KPL || pw_pass + 1 < npass)
                    eval_unit<N, KPL, HERM, VEC, decltype(no_mid)&, PK, 32>(a, mybuf + (size_t)half * MNN, tab_l, fm, seeds, seeds, 2, pw_pass * (32 * KPL),
                                                                            col, line, no_mid, half * (int)a.H.tile, half * (int)a.E.tile,
                                                                            half == 0 || k2 + 1 < a.npt, mt);
                else
                    eval_unit<N, KT, HERM, VEC, decltype(no_mid)&, PK, 32>(a, mybuf + (size_t)half * MNN, tab_l, fm, seeds_t, seeds_t, 2, pw_pass * (32 * KPL),
                                                                           col, line, no_mid, half * (int)a.H.tile, half * (int)a.E.tile,
                                                                           half == 0 || k2 + 1 < a.npt, mt);
                return;
            }
            // seeds of pass 0, read when it is the only pass: then it is the last one, of KT rounds
            int iz0[KPL], iw0[KPL], izt[KT], iwt[KT];
#pragma unroll
            for (int j = 0; j < KPL; ++j) {
                const int i1 = col + 32 * j;
                iz0[j] = i1 < a.npt ? i1 : 0;
                iw0[j] = (int)(((unsigned)fm * (unsigned)iz0[j]) % (unsigned)a.npt);
                if (j < KT) {
                    izt[j] = iz0[j];
                    iwt[j] = iw0[j];
                }
            }
            const int off_h = half * (int)a.H.tile, off_e = half * (int)a.E.tile;  // eval_route: the tiles fit 31 bits
            int cur = 0, pass = 0;
            while (k2 < a.npt) {
                // the next unit is the same pair again (its sets stay where they are) or the wave's next pair
                const bool last_pass = pass + 1 >= npass;
                const int nk2 = last_pass ? k2 + 2 * kstride : k2;
                const bool contract_next = last_pass && nk2 < a.npt;
                wave_lds_sync();
                // (kept inline, so the phases stay in registers)
                auto mid_fn = [&]() __attribute__((always_inline)) {
                    if (contract_next) {
                        // the LDS addresses of the contraction are formed here, from a lane index the compiler cannot see
                        // through: hoisted out of the work loop they were spilled to scratch at three waves per SIMD
                        int ln = lane;
                        asm volatile("" : "+v"(ln));
                        double2* const dst = mybuf + (size_t)(cur ^ 1) * 2 * MNN;
                        load_line_phases(as_const(a.phs2 + (int64_t)nk2 * a.M2), ph);
                        contract_line_m(a.M2, s2, ph, dst, MNN, ln);
                        load_line_phases(as_const(a.phs2 + (int64_t)min(nk2 + 1, a.npt - 1) * a.M2), ph);
                        contract_line_m(a.M2, s2, ph, dst + MNN, MNN, ln);
                    }
                };
                const double2* const c1 = mybuf + (size_t)(2 * cur + half) * MNN;
                const int64_t line = (int64_t)k3 * a.npt + k2;
                const bool on = half == 0 || k2 + 1 < a.npt;
                MirrorTo mt;
                if (mk3 >= 0) {
                    mt.line = (int64_t)mk3 * a.npt;
                    mt.t0 = k2 ? a.npt - k2 : 0;
                    mt.t1 = k2 + 1 < a.npt ? a.npt - k2 - 1 : 0;  // (a half without a line: nothing is stored)
                }
                if constexpr (KT == KPL) {
                    eval_unit<N, KPL, HERM, VEC, decltype(mid_fn)&, PK, 32>(a, c1, tab_l, fm, iz0, iw0, npass, pass * (32 * KPL), col, line, mid_fn,
                                                                            off_h, off_e, on, mt);
                } else if (!last_pass) {  // nothing to contract before the pair's last pass
                    auto no_mid = []() {};
                    eval_unit<N, KPL, HERM, VEC, decltype(no_mid)&, PK, 32>(a, c1, tab_l, fm, iz0, iw0, npass, pass * (32 * KPL), col, line, no_mid,
                                                                            off_h, off_e, on, mt);
                } else {
                    eval_unit<N, KT, HERM, VEC, decltype(mid_fn)&, PK, 32>(a, c1, tab_l, fm, izt, iwt, npass, pass * (32 * KPL), col, line, mid_fn,
                                                                           off_h, off_e, on, mt);
                }
                if (last_pass) cur ^= 1;
                pass = last_pass ? 0 : pass + 1;
                k2 = nk2;
            }
            return;
        }
        int iz0[KPL], iw0[KPL];
#pragma unroll
        for (int j = 0; j < KPL; ++j) {
            const int i1 = lane + 64 * j;
            iz0[j] = i1 < a.npt ? i1 : 0;
            iw0[j] = (int)(((unsigned)fm * (unsigned)iz0[j]) % (unsigned)a.npt);
        }
        int cur = 0, pass = 0;
        while (k2 < a.npt) {
            // the next unit is the same line again (its set stays where it is) or the wave's next line
            const bool last_pass = pass + 1 >= npass;
            const int nk2 = last_pass ? k2 + kstride : k2;
            const bool contract_next = last_pass && nk2 < a.npt;
            wave_lds_sync();
            auto mid_fn = [&]() {
                if (contract_next) {
                    load_line_phases(as_const(a.phs2 + (int64_t)nk2 * a.M2), ph);
                    contract_line_m(a.M2, s2, ph, mybuf + (size_t)(cur ^ 1) * MNN, MNN, lane);
                }
            };
            MirrorTo mt;
            if (mk3 >= 0) mt.line = (int64_t)mk3 * a.npt + (k2 ? a.npt - k2 : 0);
            eval_unit<N, KPL, HERM, VEC, decltype(mid_fn)&, PK>(a, mybuf + (size_t)cur * MNN, tab_l, fm, iz0, iw0, npass, pass * (64 * KPL), lane,
                                                                (int64_t)k3 * a.npt + k2, mid_fn, 0, 0, true, mt);
            if (last_pass) cur ^= 1;
            pass = last_pass ? 0 : pass + 1;
            k2 = nk2;
        }
        return;
    }
    for (int i = threadIdx.x; i < a.npt; i += 256) tab_l[i] = a.tab[i];
    __syncthreads();
    const int64_t lstride = (int64_t)gridDim.x * 4;
    int64_t line = (int64_t)blockIdx.x * 4 + wave;
    if (line >= a.nlines) return;
    // stage the first line
    {
        const double2* __restrict__ src = a.src + line * MNN;
#pragma unroll
        for (int t = 0; t < EVAL_MAX_MNN / 64; ++t) {
            const int idx = lane + 64 * t;
            if (idx < MNN) mybuf[idx] = stage(src[idx], idx);
        }
    }
    // table indices of z and of the seed w = z^first for the nodes of pass 0
    int iz0[KPL], iw0[KPL];
#pragma unroll
    for (int j = 0; j < KPL; ++j) {
        const int i1 = lane + 64 * j;
        iz0[j] = i1 < a.npt ? i1 : 0;
        iw0[j] = (int)(((unsigned)fm * (unsigned)iz0[j]) % (unsigned)a.npt);
    }
    int cur = 0, pass = 0;
    while (line < a.nlines) {
        // fetch the next unit's coefficients into registers (the same line again if it has more passes)
        const bool last_pass = pass + 1 >= npass;
        const int64_t nline = last_pass ? line + lstride : line;
        const bool have_next = nline < a.nlines;
        double2 pre[EVAL_MAX_MNN / 64];
        {
            const double2* __restrict__ src = a.src + (have_next ? nline : line) * MNN;
#pragma unroll
            for (int t = 0; t < EVAL_MAX_MNN / 64; ++t) {
                const int idx = lane + 64 * t;
                pre[t] = src[idx < MNN ? idx : MNN - 1];  // unconditional: no select waits on the data
            }
        }
        wave_lds_sync();
        auto mid_fn = [&]() {
            // The one wait of the loop body: the fetched registers are consumed here, unconditionally and
            // before this unit's stores are issued (the asm pins the point; nothing is hoisted above it).
#pragma unroll
            for (int t = 0; t < EVAL_MAX_MNN / 64; ++t) asm volatile("" : "+v"(pre[t].x), "+v"(pre[t].y));
            if (have_next) {
                double2* dst = mybuf + (size_t)(cur ^ 1) * MNN;
#pragma unroll
                for (int t = 0; t < EVAL_MAX_MNN / 64; ++t) {
                    const int idx = lane + 64 * t;
                    if (idx < MNN) dst[idx] = stage(pre[t], idx);
                }
            }
        };
        MirrorTo mt;
        if constexpr (MIR) {  // a.nlines: the lines of the planes k3 <= npt / 2, fewer than 2^31 (eval_mirror_taken)
            const unsigned k3 = (unsigned)line / (unsigned)a.npt, k2 = (unsigned)line - k3 * (unsigned)a.npt;
            if (k3 != 0 && 2 * (int)k3 != a.npt) mt.line = (int64_t)(a.npt - (int)k3) * a.npt + (k2 ? a.npt - (int)k2 : 0);
        }
        eval_unit<N, KPL, HERM, VEC, decltype(mid_fn)&, PK>(a, mybuf + (size_t)cur * MNN, tab_l, fm, iz0, iw0, npass, pass * (64 * KPL), lane, line,
                                                            mid_fn, 0, 0, true, mt);
        cur ^= 1;
        pass = last_pass ? 0 : pass + 1;
        line = nline;
    }
}

// Fallback for coefficient sets too large for the LDS staging above: wave-uniform scalar loads.
template <int N>
__global__ __launch_bounds__(256) void eval_grid_kernel_scalar(EvalArgs a) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int fm = a.first % a.npt;
    if (fm < 0) fm += a.npt;
    for (int64_t line = (int64_t)blockIdx.x * 4 + wave; line < a.nlines; line += (int64_t)gridDim.x * 4) {
        const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)(line & 0xffffffffu));
        const unsigned hi = __builtin_amdgcn_readfirstlane((unsigned)((unsigned long long)line >> 32));
        const int64_t line_u = (int64_t)(((unsigned long long)hi << 32) | lo);
        cptr_t c1 = as_const(a.src + line_u * ((int64_t)a.M * N * N));
        for (int i0 = 0; i0 < a.npt; i0 += 64) {
            const int i1 = i0 + lane;
            if (i1 < a.npt) {
                const double2 z = a.tab[i1];
                const double2 w = a.tab[(int)(((int64_t)fm * i1) % a.npt)];
                CMat<N> H;
                series_lane<N>(c1, a.M, a.first, z.x, z.y, w.x, w.y, a.deriv != 0, H);
                eval_epilogue<N>(a, H, line_u, i1);
            }
        }
    }
}

template <int N>
__global__ __launch_bounds__(256) void eval_node_kernel(EvalArgs a) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= a.nk) return;
    const int64_t slot = a.parents ? a.parents[k] : 0;
    cptr_t c1 = as_const(a.src + slot * ((int64_t)a.M * N * N));
    double zr, zi, wr, wi;
    if (a.x == nullptr) {
        const int i1 = a.gi[k];
        int fm = a.first % a.npt;
        if (fm < 0) fm += a.npt;
        const double2 z = a.tab[i1];
        const double2 w = a.tab[(int)(((int64_t)fm * i1) % a.npt)];
        zr = z.x;
        zi = z.y;
        wr = w.x;
        wi = w.y;
    } else {
        const double xx = a.x[k] * a.inv_period;
        sincospi(2.0 * xx, &zi, &zr);
        sincospi(2.0 * ((double)a.first * xx), &wi, &wr);
    }
    CMat<N> H;
    series_lane<N>(c1, a.M, a.first, zr, zi, wr, wi, a.deriv != 0, H);
    const int ll = a.H.base ? a.H.line_len : (a.E.base ? a.E.line_len : a.U.line_len);
    const int64_t line = k / ll;
    eval_epilogue<N>(a, H, line, (int)(k - line * ll));
}

// ---- from run-time values to an instance -----------------------------------------------------------------------------
// f(std::integral_constant<int, v>{}) for LO <= v <= HI, nothing beyond
template <int LO, int HI, class F>
static void with_int(int v, F&& f) {
    if constexpr (LO <= HI) {
        if (v == LO)
            f(std::integral_constant<int, LO>{});
        else
            with_int<LO + 1, HI>(v, f);
    }
}
// f(std::bool_constant<p>{}, std::bool_constant<q>{})
template <class F>
static void with_flags(bool p, bool q, F&& f) {
    if (p)
        q ? f(std::true_type{}, std::true_type{}) : f(std::true_type{}, std::false_type{});
    else
        q ? f(std::false_type{}, std::true_type{}) : f(std::false_type{}, std::false_type{});
}

// The instances of eval_grid_kernel that are built -- the ones eval_route can ask for.  Eigenvectors: the streamed mapping of
// whole matrices.  General series have no packed sets, no mirror and no pass per wave.  The pair mappings have one pass
// length per band count (eval_pair_rounds) and every shorter last pass.
template <int N, int KPL, int KT, bool HERM, bool VEC, bool PK, EvalMapping MAP, bool MIR>
constexpr bool eval_instance_built() {
    if (VEC) return MAP == EvalMapping::streamed && !HERM && !PK && !MIR && KT == KPL;
    if (!HERM && (PK || MIR || MAP == EvalMapping::fused_passwave)) return false;
    if (MAP == EvalMapping::streamed || MAP == EvalMapping::fused_lines) return KT == KPL;
    return KPL == eval_pair_rounds(N, HERM) && KT <= KPL;
}

// f(EvalCfg<...>{}) for the instance of a route; false where none is built
template <class F>
static bool with_eval_cfg(int n, const EvalRoute& r, F&& f) {
    bool found = false;
    with_int<1, 4>(n, [&](auto n_) {
        with_int<1, 3>(r.kp, [&](auto kp_) {
            with_int<1, 3>(r.kt, [&](auto kt_) {
                with_int<(int)EvalMapping::streamed, (int)EvalMapping::fused_passwave>((int)r.mapping, [&](auto map_) {
                    with_flags(r.herm, r.vec, [&](auto herm_, auto vec_) {
                        with_flags(r.pk, r.mirror, [&](auto pk_, auto mir_) {
                            constexpr int N = decltype(n_)::value, KPL = decltype(kp_)::value, KT = decltype(kt_)::value;
                            constexpr bool HERM = decltype(herm_)::value, VEC = decltype(vec_)::value, PK = decltype(pk_)::value,
                                           MIR = decltype(mir_)::value;
                            constexpr EvalMapping MAP = (EvalMapping) decltype(map_)::value;
                            if constexpr (eval_instance_built<N, KPL, KT, HERM, VEC, PK, MAP, MIR>()) {
                                f(EvalCfg<N, KPL, KT, HERM, VEC, PK, MAP, MIR>{});
                                found = true;
                            }
                        });
                    });
                });
            });
        });
    });
    return found;
}

EvalSwitches eval_switches() {
    EvalSwitches sw;
    sw.pairs = abz_switch(SW_EVAL_PAIRS);
    sw.mirror = abz_switch(SW_EVAL_MIRROR);
    sw.passwave = abz_switch(SW_EVAL_PASSWAVE);
    sw.packed = abz_switch(SW_EVAL_PACKED);
    return sw;
}

static EvalPlanes eval_planes(const PlaneView& v) {
    EvalPlanes p;
    p.present = v.base != nullptr;
    p.row = v.row;
    p.tile = v.tile;
    p.compact = v.compact != 0;
    return p;
}

static void count_launch(abz_ctx* ctx, int slot) {
    if (ctx->prof & (1u << slot)) ctx->prof_slots[slot].launches += 1;
}

int launch_eval(abz_ctx* ctx, const EvalSpec& es) {
    if (es.n > 4) {
        GenSpec gs;
        gs.Uplanes = es.U;
        gs.herm = es.herm && !es.deriv;
        gs.n = es.n;
        gs.M = es.M;
        gs.first = es.first;
        gs.npt = es.npt;
        gs.d = 0;
        gs.period = es.period;
        gs.src = es.src;
        gs.grid = es.grid;
        gs.parents = es.parents;
        gs.run_start = es.run_start;
        gs.nruns = es.nruns;
        gs.gi = es.gi;
        gs.x = es.x;
        gs.tab = es.tab;
        gs.deriv = es.deriv;
        gs.nnodes = es.grid ? es.nlines * es.npt : es.nk;
        gs.Hplanes = es.H;
        gs.Eplanes = es.E;
        gs.Haos = nullptr;
        gs.Eaos = nullptr;
        gs.integrand = ABZ_F_ONE;
        for (int i = 0; i < 4; ++i) gs.params[i] = 0.0;
        gs.sweep_dev = nullptr;
        gs.sweep0 = 0.0;
        gs.n_sweep = 0;
        gs.values = nullptr;
        return launch_gen_nodes(ctx, gs);
    }
    if (es.n < 1) {
        set_error("n = %d bands: only n <= 4 is built in this round", es.n);
        return ABZ_ERR_UNSUPPORTED;
    }
    EvalArgs a;
    a.src = es.src;
    a.tab = es.tab;
    a.parents = es.parents;
    a.gi = es.gi;
    a.x = es.x;
    a.H = es.H;
    a.E = es.E;
    a.U = es.U;
    a.nlines = es.nlines;
    a.nk = es.nk;
    a.line0 = 0;
    a.M = es.M;
    a.first = es.first;
    a.npt = es.npt > 0 ? es.npt : 1;
    a.deriv = es.deriv ? 1 : 0;
    a.herm = (es.herm && !es.deriv) ? 1 : 0;
    a.nt = 0;
    a.pk = 0;
    a.inv_period = 1.0 / es.period;
    ProfScope ps(ctx, ABZ_K_EVAL);
    if (!es.grid) {
        if (es.nk == 0) return ABZ_OK;
        with_int<1, 4>(es.n, [&](auto n_) {
            launch(ctx, eval_node_kernel<decltype(n_)::value>, dim3((unsigned)eval_cdiv(es.nk, 256)), dim3(256), 0, a);
        });
        ABZ_HIP(hipGetLastError());
        return ABZ_OK;
    }
    if (es.nlines == 0) return ABZ_OK;
    EvalShape sh;
    sh.n = es.n;
    sh.M = es.M;
    sh.M2 = es.M2;
    sh.npt = es.npt;
    sh.nlines = es.nlines;
    sh.herm = es.herm;
    sh.real_coef = es.real_coef;
    sh.deriv = es.deriv;
    sh.packed = es.packed;
    sh.fused = es.src2 != nullptr;
    sh.H = eval_planes(es.H);
    sh.E = eval_planes(es.E);
    sh.U = eval_planes(es.U);
    sh.whole_grid3 = es.whole_grid3;
    sh.velocity = es.velocity;
    const EvalRoute r = eval_route(sh, eval_switches());
    a.nt = r.nt ? 1 : 0;
    a.pk = r.pk ? 1 : 0;
    a.mirror = r.mirror ? 1 : 0;
    a.nlines = r.nlines;
    a.src2 = es.src2;
    a.phs2 = es.phs2;
    a.M2 = es.M2;
    a.bpk = r.bpk;
    if (r.mapping == EvalMapping::unsupported) {
        set_error("eval: fused contraction unsupported (n = %d, %d numbers per line, M2 = %d, npt = %d)", es.n, r.mnn, es.M2, es.npt);
        return ABZ_ERR_UNSUPPORTED;
    }
    if (r.mapping == EvalMapping::scalar) {
        with_int<1, 4>(es.n, [&](auto n_) { launch(ctx, eval_grid_kernel_scalar<decltype(n_)::value>, dim3(r.grid_x), dim3(256), 0, a); });
        ABZ_HIP(hipGetLastError());
        return ABZ_OK;
    }
    if (r.mapping != EvalMapping::streamed) count_launch(ctx, ABZ_K_EVAL_FUSED);
    if (r.mapping == EvalMapping::fused_passwave) count_launch(ctx, ABZ_K_EVAL_PASSWAVE);
    const bool built = with_eval_cfg(es.n, r, [&](auto cfg) {
        launch(ctx, eval_grid_kernel<decltype(cfg)>, dim3(r.grid_x, r.grid_y), dim3(256), r.lds, a);
    });
    if (!built) {  // a route that eval_instance_built does not know: a missing kernel is an error
        set_error("eval: no kernel instance for the route (n = %d, mapping %d, passes of %d and %d)", es.n, (int)r.mapping, r.kp, r.kt);
        return ABZ_ERR_UNSUPPORTED;
    }
    ABZ_HIP(hipGetLastError());
    return ABZ_OK;
}

}  // namespace abz
