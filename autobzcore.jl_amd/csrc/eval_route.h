// The route of a grid-mode Fourier evaluation (eval_grid_kernel, kernels_eval.hip): which instance runs, on what launch grid,
// with how much LDS.  Every selection rule of the family is here and nowhere else; launch_eval reads an EvalRoute and
// launches, rule_fill asks the same header for the kernel-side limits.  Nothing of HIP is needed here
// (tests/c/eval_route_main.cpp checks the function against a recorded table on the CPU).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace abz {

constexpr int EVAL_MAX_MNN = 256;           // complex coefficients per line held in LDS (M * N * N)
constexpr int ABZ_CONTRACT_GRID_MAXM = 16;  // most coefficients of a contracted variable (launch_contract_grid; fused: M2)
constexpr size_t EVAL_LDS_BYTES = 64 * 1024;
constexpr size_t EVAL_CPLX = 16;            // sizeof(double2)

// what the decision reads of a rule array (PlaneView)
struct EvalPlanes {
    bool present = false;
    int row = 0;       // padded row length
    int64_t tile = 0;  // doubles from one line to the next
    bool compact = false;
};

struct EvalShape {
    int n = 0;           // bands, 1 ... 4
    int M = 0, M2 = 0;   // coefficients of the innermost variable and of variable 2
    int npt = 0;
    int64_t nlines = 0;
    bool herm = false;       // the series is Hermitian
    bool real_coef = false;  // ... and H_R is real: H(-k) = conj H(k)
    bool deriv = false;
    bool packed = false;     // the level-1 (fused: level-2) sets are packed Hermitian sets (packed_herm.h)
    bool fused = false;      // level-2 sets are given (EvalSpec::src2): the kernel contracts variable 2 itself
    EvalPlanes H, E, U;
    // the caller's facts
    bool whole_grid3 = false;  // a whole 3-D grid (a slab's mirror planes belong to another rank)
    bool velocity = false;     // the rule wants velocities
};

// ABZ_EVAL_PAIRS, ABZ_EVAL_MIRROR, ABZ_EVAL_PASSWAVE, ABZ_EVAL_PACKED (abz_internal.h: Switch); the caller fills them in
struct EvalSwitches {
    int pairs = 1, mirror = 1, passwave = 1, packed = 1;
};

enum class EvalMapping {
    unsupported,     // fused contraction asked for where the kernel cannot do it
    scalar,          // eval_grid_kernel_scalar: coefficient sets too large for LDS
    streamed,        // level-1 sets from memory, one line per wave
    fused_lines,     // variable 2 contracted in the kernel, one line per wave
    fused_pairs,     // ... one line per half-wave, a pair of lines per wave
    fused_passwave,  // ... one pass of a pair per wave
};

struct EvalRoute {
    EvalMapping mapping = EvalMapping::unsupported;
    int mnn = 0;      // numbers per line
    int kpl = 1;      // nodes per lane of the 64-lane mapping (eval_kpl)
    int kp = 1;       // rounds of a pass: kpl, pair mappings eval_pair_rounds
    int kt = 1;       // rounds of the last pass: kp, pair mappings 1 ... kp
    int npass = 1;    // passes of a line or pair
    int bpk = 0;      // fused: blocks per outermost index
    unsigned grid_x = 0, grid_y = 1;
    size_t lds = 0;
    int occ = 0;      // waves per SIMD the register allocator is asked for (eval_occupancy; the scalar kernel has no hint)
    bool herm = false;    // the Hermitian instance: upper triangle only
    bool vec = false;     // the eigenvector instance
    bool mirror = false;  // planes k3 <= npt / 2 evaluated, the rest stored as their mirror images
    bool nt = false;      // non-temporal stores
    bool pk = false;      // packed sets
    int64_t nlines = 0;   // lines evaluated
};

inline int64_t eval_cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

// numbers per line: packed Hermitian sets (packed_herm.h: Pk<n>::size((M - 1) / 2)) or M n n
inline int eval_line_elems(int n, int M, bool packed) {
    return packed ? n * (n + 1) / 2 + ((M - 1) / 2) * n * n : M * n * n;
}

// nodes per lane: minimise lane-rounds per line, ceil(npt / (64 kpl)) * kpl, weighted by the LDS
// operand reads that are shared by the kpl nodes of a lane (200 points: 2 x 2 rounds, not 2 x 3)
inline int eval_kpl(int npt, int kmin = 1) {
    int kpl = kmin;
    double best = 1e30;
    for (int k = kmin; k <= 3; ++k) {
        const double cost = (double)(eval_cdiv(npt, 64 * k) * k) * (1.0 + 0.3 / k);
        if (cost < best - 1e-12) {
            best = cost;
            kpl = k;
        }
    }
    return kpl;
}

// Rounds of 32 columns in a pass of the pair mapping -- the most the instance holds without scratch in its work loop: 3,
// with 4 bands 2, non-Hermitian 1
constexpr int eval_pair_rounds(int n, bool herm) { return n < 4 ? 3 : (herm ? 2 : 1); }

// waves per SIMD the register allocator is asked for: 3 on the Hermitian 3-band paths (2 and 4 measured
// slower there), 2 elsewhere
constexpr int eval_occupancy(int n, bool herm) { return herm && n == 3 ? 3 : 2; }

// bytes a launch writes, padding included, over `tiles` lines (or tiles of 64 nodes)
inline double eval_out_bytes(const EvalShape& s, int64_t tiles) {
    const EvalPlanes& pv = s.H.present ? s.H : s.E;
    const double planes = (s.H.present ? (s.H.compact ? 1.0 : 2.0) * s.n * s.n : 0.0) + (s.E.present ? (double)s.n : 0.0) +
                          (s.U.present ? 2.0 * s.n * s.n : 0.0);
    return 8.0 * planes * (double)pv.row * (double)tiles;
}
// streaming stores once the values written by a launch exceed the 256 MB Infinity Cache
// (npt = 100, 168 MB: 7 % slower with them; 150, 605 MB: 19 % faster)
inline bool eval_nontemporal(const EvalShape& s, int64_t tiles) { return eval_out_bytes(s, tiles) > 256.0 * 1024 * 1024; }

// LDS of the staged paths: four waves' buffers of `sets` line sets each, an LDS copy of the phase table (fm * i1 < npt^2 must
// fit 32 bits) and, fused, the level-2 set of one outermost index
inline size_t eval_lds_bytes(int mnn, int npt, int sets, int M2 = 0) {
    return EVAL_CPLX * ((size_t)M2 * mnn + 4 * (size_t)sets * mnn + (size_t)npt);
}
inline bool eval_staged_supported(int n, int64_t mnn, int npt) {
    return n >= 1 && n <= 4 && mnn >= 1 && mnn <= EVAL_MAX_MNN && npt >= 1 && npt < 65536;
}

// Can the grid kernel take packed Hermitian level-1 sets (packed_herm.h)?  Same limits as its LDS-staged path.
inline bool eval_packed_supported(int n, int M, int npt, const EvalSwitches& sw) {
    if (!sw.packed || n < 1 || n > 4 || (M & 1) == 0) return false;
    const int P = eval_line_elems(n, M, true);
    return eval_staged_supported(n, P, npt) && eval_lds_bytes(P, npt, 2) <= EVAL_LDS_BYTES;
}

// Can the grid kernel contract variable 2 itself (EvalSpec::src2)?  Its LDS-staged path with the level-2 set of one
// outermost index next to the four waves' double buffers and the phase table; `mnn` numbers per line.
// `pairs`: the pair mapping (one line per half-wave), whose waves hold two lines' sets in each buffer.
inline bool eval_fused_supported(int n, int64_t mnn, int M2, int npt, bool pairs = false) {
    return eval_staged_supported(n, mnn, npt) && M2 >= 1 && M2 <= ABZ_CONTRACT_GRID_MAXM &&
           eval_lds_bytes((int)mnn, npt, pairs ? 4 : 2, M2) <= EVAL_LDS_BYTES;
}

// Can a launch evaluate the planes k3 <= npt / 2 alone and store the rest as their mirror images?  A whole 3-D grid, values /
// eigenvalues of a real Hermitian series; the mirrored row is addressed from the first line of its plane by a 32-bit lane
// offset.
// Size rule (profiles/eval_mirror_trace_gaps.txt): by the bytes the launch writes, padding
// included.  Every measured shape up to 597 MB was faster mirrored (3 and 4 bands, both layouts: 3-32 %), 605 MB tied
// (+2 %) and 665 MB and more lost 9-50 % with 3 bands -- the mirrored stores are temporal, and beyond that they no
// longer leave L2 as whole lines.  (4 bands still won 15 % at 814 MB and lost at 1331 MB; the limit is not tuned per
// band count.)  ABZ_EVAL_MIRROR=2 takes the route wherever it is supported.
inline bool eval_mirror_taken(const EvalShape& s, const EvalSwitches& sw) {
    if (!(s.herm && s.real_coef && s.whole_grid3 && !s.deriv && !s.U.present && !s.velocity)) return false;
    if (!(sw.mirror >= 2 || (sw.mirror == 1 && eval_out_bytes(s, s.nlines) <= 600e6))) return false;
    if (s.n < 1 || s.n > 4 || s.npt < 1 || s.npt >= 65536 || s.nlines != (int64_t)s.npt * s.npt || s.nlines >= INT32_MAX) return false;
    for (const EvalPlanes* v : {&s.H, &s.E})
        if (v->present && ((int64_t)s.npt * v->tile + v->row >= INT32_MAX || v->tile < 0)) return false;
    return true;
}

inline EvalRoute eval_route(const EvalShape& s, const EvalSwitches& sw) {
    EvalRoute r;
    const int npt = s.npt > 0 ? s.npt : 1;
    r.herm = s.herm && !s.deriv;
    r.nt = eval_nontemporal(s, s.nlines);
    r.pk = s.packed && r.herm && !s.U.present;
    r.nlines = s.nlines;
    r.mnn = eval_line_elems(s.n, s.M, r.pk);
    r.kpl = r.kp = r.kt = eval_kpl(npt);
    r.npass = (int)eval_cdiv(npt, 64 * r.kpl);
    // Workgroups: 8 per CU up to ~140^3, 16 per CU beyond (3 bands: npt 150 0.1133 -> 0.1101 ms on a fast box,
    // 0.1234 -> 0.1175 on a slow one; 200 -6 %, 250 -15 %, 300 -3 %, 500 -6 %; 110 / 128 are 3-5 % better with 8 per
    // CU, 180 and 400 lose 2-3 % with 16); compact H planes: 24 per CU -- at 150^3 one line per wave -- measured
    // 1.5 % better than 16, the same at 200^3
    const int64_t quads = eval_cdiv(s.nlines, 4);
    const int64_t blocks = std::min<int64_t>(quads, quads < 5000 ? 256 * 8 : (s.H.compact ? 256 * 24 : 256 * 16));
    const size_t lds = eval_lds_bytes(r.mnn, npt, 2);
    if (!s.fused) {
        if (!(eval_staged_supported(s.n, r.mnn, npt) && lds <= EVAL_LDS_BYTES)) {
            // the scalar fallback kernel evaluates every line
            r.mapping = EvalMapping::scalar;
            r.grid_x = (unsigned)blocks;
            return r;
        }
        r.mapping = EvalMapping::streamed;
        r.vec = s.U.present;
        r.herm = r.herm && !r.vec;  // the eigenvector instance evaluates whole matrices
        r.occ = eval_occupancy(s.n, r.herm);
        // mirror: the lines of the planes k3 <= npt / 2, which come first
        r.mirror = eval_mirror_taken(s, sw);
        if (r.mirror) r.nlines = (int64_t)(npt / 2 + 1) * npt;
        r.grid_x = (unsigned)std::min<int64_t>(blocks, eval_cdiv(r.nlines, 4));
        r.lds = lds;
        return r;
    }
    // fused last contraction: whole blocks per outermost index, about the block count chosen above (150^3: one
    // line per wave, 38 blocks for each of the 150 indices)
    if (s.deriv || s.U.present || !eval_fused_supported(s.n, r.mnn, s.M2, npt) || s.nlines % npt != 0 || s.nlines / npt > 65535) return r;
    r.occ = eval_occupancy(s.n, r.herm);
    const int64_t gcnt = s.nlines / npt;
    // mirror: the launch grid's rows are the planes k3 <= npt / 2; blocks per plane as for the whole grid
    r.mirror = eval_mirror_taken(s, sw);
    r.grid_y = r.mirror ? (unsigned)(npt / 2 + 1) : (unsigned)gcnt;
    // ... then the fewest blocks with the same number of lines per wave: every wave of an index gets its share
    // (100 points: 21 blocks would give 16 of 84 waves a second line; 13 give 48 of 52 two)
    auto blocks_per_index = [&](int64_t units) {
        const int64_t b = std::max<int64_t>(1, std::min<int64_t>(eval_cdiv(units, 4), eval_cdiv(blocks, gcnt)));
        return (int)eval_cdiv(units, 4 * eval_cdiv(units, 4 * b));
    };
    // Pair mapping (one line per half-wave): the same count over rounds of 32 lanes, for two lines at once.  Its
    // passes are of kp rounds (eval_pair_rounds) and the last pass of the rest, kt, so a pair costs ceil(npt / 32)
    // lane-rounds.  It is taken where that is fewer than two lines of the 64-lane mapping cost (150 points: 5 against
    // 2 x 3); ties keep the 64-lane mapping (measured slower or equal there: +6 % at 64 and 250 points), and so do
    // non-Hermitian series (3 bands: +7 % at 80 points, +4 % at 200, -2 % at 150).
    // ABZ_EVAL_PAIRS: 0 never, 2 wherever the kernel supports it.
    const int rounds = (int)eval_cdiv(npt, 32);
    const bool pairs = sw.pairs != 0 && eval_fused_supported(s.n, r.mnn, s.M2, npt, true) && s.H.tile < INT32_MAX && s.E.tile < INT32_MAX &&
                       (sw.pairs >= 2 || (r.herm && rounds < 2 * r.npass * r.kpl));
    if (!pairs) {
        r.mapping = EvalMapping::fused_lines;
        r.bpk = blocks_per_index(npt);
        r.lds = eval_lds_bytes(r.mnn, npt, 2, s.M2);
    } else {
        r.kp = eval_pair_rounds(s.n, r.herm);
        r.npass = (int)eval_cdiv(rounds, r.kp);
        r.kt = rounds - (r.npass - 1) * r.kp;  // 1 ... kp
        const int64_t npairs = eval_cdiv(npt, 2);
        // One pass of a pair per wave: Hermitian series whose pairs take 2 or 4 passes, so that a block holds whole pairs;
        // one pass is the pair instance as it is, three passes keep it.  Selection rule (DESIGN section 9 item 1,
        // profiles/eval_passwave_trace_gaps.txt): pairs of two passes -- 97 ... 192 points, with 4 bands 65 ... 128.  Every
        // measured shape on which pairs are taken by default was faster than a pair per wave: SVO 129 ... 160 points 6-17 %,
        // 4 bands real 70 ... 96 points 12-22 %, a complex Hermitian 3-band series at 150 points (not mirrored) 3.6 %.
        // Pairs of four passes (4 bands, 193 ... 256 points) are not measured and run under ABZ_EVAL_PASSWAVE=2 only.
        const bool passwave = r.herm && ((sw.passwave >= 1 && r.npass == 2) || (sw.passwave >= 2 && r.npass == 4));
        if (passwave) {
            r.mapping = EvalMapping::fused_passwave;
            r.bpk = (int)eval_cdiv(npairs * r.npass, 4);
            // one buffer of two line sets per wave: the room of the 64-lane mapping's two buffers
            r.lds = eval_lds_bytes(r.mnn, npt, 2, s.M2);
        } else {
            r.mapping = EvalMapping::fused_pairs;
            // blocks per index by the rule above, counted in pairs (150 points: 19 blocks, one pair per wave; two pairs
            // per wave measured 9 % slower there and 7 % at 200 points)
            r.bpk = blocks_per_index(npairs);
            r.lds = eval_lds_bytes(r.mnn, npt, 4, s.M2);
        }
    }
    r.grid_x = (unsigned)r.bpk;
    return r;
}

}  // namespace abz
