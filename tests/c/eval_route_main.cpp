// eval_route (csrc/eval_route.h) against a table of shapes and the routes that the launcher took for them before the
// decisions moved into one function.  The expected rows were recorded from that earlier launch code (which instance it
// launched, on what grid, with how much LDS, which counters it bumped), not from eval_route; a sweep over 1 ... 4 bands,
// 1 ... 300 points, every kind of series, layout and switch value compared the two field by field when the function was
// written (1555200 cases, no mismatch).  Needs nothing of HIP: g++ -std=c++17 -Wall -Wextra -Werror.
#include "../../autobzcore.jl_amd/csrc/eval_route.h"

#include <cstdio>

using abz::EvalRoute;
using M = abz::EvalMapping;

// A rule build on a whole 3-D grid as rule_fill describes it to the launcher.
struct Shape {
    int n, npt;
    char series;  // 'r' real Hermitian, 'c' complex Hermitian, 'g' general
    char out;     // 'F' full H + E, 'C' compact H + E, 'E' eigenvalues only, 'U' H + E + eigenvectors (a velocity build)
    int fused;    // level-2 sets given: the kernel contracts variable 2
    int M, M2;
    int sw_pairs, sw_mirror, sw_passwave;  // ABZ_EVAL_PAIRS, ABZ_EVAL_MIRROR, ABZ_EVAL_PASSWAVE
};

struct Expected {
    M mapping;
    int mnn, kpl, kp, kt, npass, bpk;
    unsigned grid_x, grid_y;
    size_t lds;
    int occ;
    bool herm, vec, mirror, nt, pk;
    long long nlines;
};

struct Case {
    const char* what;
    Shape shape;
    Expected want;
};

static const Case CASES[] = {
    {"npt 150: the benchmark's launch",
     {3, 150, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_passwave, 24, 3, 3, 2, 2, 38, 38u, 76u, 7392, 3, true, false, true, true, true, 22500LL}},
    {"npt 128: the tie keeps the 64-lane mapping",
     {3, 128, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_lines, 24, 2, 2, 2, 1, 16, 16u, 65u, 7040, 3, true, false, true, false, true, 16384LL}},
    {"npt 129: pairs, one pass per wave",
     {3, 129, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_passwave, 24, 3, 3, 2, 2, 33, 33u, 65u, 7056, 3, true, false, true, false, true, 16641LL}},
    {"npt 100: lines, 13 blocks per index",
     {3, 100, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_lines, 24, 2, 2, 2, 1, 13, 13u, 51u, 6592, 3, true, false, true, false, true, 10000LL}},
    {"npt 193: pairs of three passes",
     {3, 193, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_pairs, 24, 2, 3, 1, 3, 25, 25u, 193u, 11152, 3, true, false, false, true, true, 37249LL}},
    {"npt 193, ABZ_EVAL_PASSWAVE=2: three passes keep the pair per wave",
     {3, 193, 'r', 'C', 1, 5, 5, 1, 1, 2},
     {M::fused_pairs, 24, 2, 3, 1, 3, 25, 25u, 193u, 11152, 3, true, false, false, true, true, 37249LL}},
    {"npt 24, ABZ_EVAL_PAIRS=2: pairs of one pass",
     {3, 24, 'r', 'C', 1, 5, 5, 2, 1, 1},
     {M::fused_pairs, 24, 1, 3, 1, 1, 3, 3u, 13u, 8448, 3, true, false, true, false, true, 576LL}},
    {"npt 24, ABZ_EVAL_PAIRS=2, ABZ_EVAL_PASSWAVE=2: one pass has no pass per wave",
     {3, 24, 'r', 'C', 1, 5, 5, 2, 1, 2},
     {M::fused_pairs, 24, 1, 3, 1, 1, 3, 3u, 13u, 8448, 3, true, false, true, false, true, 576LL}},
    {"4 bands, npt 70",
     {4, 70, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_passwave, 42, 2, 2, 1, 2, 18, 18u, 36u, 9856, 2, true, false, true, false, true, 4900LL}},
    {"4 bands, npt 193: four passes, default switches",
     {4, 193, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_pairs, 42, 2, 2, 1, 4, 25, 25u, 193u, 17200, 2, true, false, false, true, true, 37249LL}},
    {"4 bands, npt 193, ABZ_EVAL_PASSWAVE=2",
     {4, 193, 'r', 'C', 1, 5, 5, 1, 1, 2},
     {M::fused_passwave, 42, 2, 2, 1, 4, 97, 97u, 193u, 11824, 2, true, false, false, true, true, 37249LL}},
    {"4 bands, npt 224: four passes, default switches",
     {4, 224, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_pairs, 42, 2, 2, 1, 4, 28, 28u, 224u, 17696, 2, true, false, false, true, true, 50176LL}},
    {"4 bands, npt 224, ABZ_EVAL_PASSWAVE=2",
     {4, 224, 'r', 'C', 1, 5, 5, 1, 1, 2},
     {M::fused_passwave, 42, 2, 2, 1, 4, 112, 112u, 224u, 12320, 2, true, false, false, true, true, 50176LL}},
    {"4 bands, npt 256: a tie, lines",
     {4, 256, 'r', 'C', 1, 5, 5, 1, 1, 2},
     {M::fused_lines, 42, 2, 2, 2, 2, 22, 22u, 256u, 12832, 2, true, false, false, true, true, 65536LL}},
    {"4 bands, npt 256, ABZ_EVAL_PAIRS=2, ABZ_EVAL_PASSWAVE=2",
     {4, 256, 'r', 'C', 1, 5, 5, 2, 1, 2},
     {M::fused_passwave, 42, 2, 2, 2, 4, 128, 128u, 256u, 12832, 2, true, false, false, true, true, 65536LL}},
    {"general 3-band series, npt 150: lines",
     {3, 150, 'g', 'F', 1, 5, 5, 1, 1, 1},
     {M::fused_lines, 45, 3, 3, 3, 1, 19, 19u, 150u, 11760, 2, false, false, false, true, false, 22500LL}},
    {"general 3-band series, npt 150, ABZ_EVAL_PAIRS=2: pairs of 3 + 2 rounds, no pass per wave",
     {3, 150, 'g', 'F', 1, 5, 5, 2, 1, 2},
     {M::fused_pairs, 45, 3, 3, 2, 2, 19, 19u, 150u, 17520, 2, false, false, false, true, false, 22500LL}},
    {"general 4-band series, npt 70, ABZ_EVAL_PAIRS=2: passes of one round",
     {4, 70, 'g', 'F', 1, 5, 5, 2, 1, 1},
     {M::fused_pairs, 80, 2, 1, 1, 3, 9, 9u, 70u, 28000, 2, false, false, false, false, false, 4900LL}},
    {"complex Hermitian, npt 150: pass per wave, not mirrored",
     {3, 150, 'c', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_passwave, 24, 3, 3, 2, 2, 38, 38u, 150u, 7392, 3, true, false, false, true, true, 22500LL}},
    {"npt 150, ABZ_EVAL_PAIRS=0: lines under the mirror",
     {3, 150, 'r', 'C', 1, 5, 5, 0, 1, 1},
     {M::fused_lines, 24, 3, 3, 3, 1, 38, 38u, 76u, 7392, 3, true, false, true, true, true, 22500LL}},
    {"npt 150, ABZ_EVAL_PASSWAVE=0: a pair per wave",
     {3, 150, 'r', 'C', 1, 5, 5, 1, 1, 0},
     {M::fused_pairs, 24, 3, 3, 2, 2, 19, 19u, 76u, 10464, 3, true, false, true, true, true, 22500LL}},
    {"npt 150, ABZ_EVAL_MIRROR=0: every plane",
     {3, 150, 'r', 'C', 1, 5, 5, 1, 0, 1},
     {M::fused_passwave, 24, 3, 3, 2, 2, 38, 38u, 150u, 7392, 3, true, false, false, true, true, 22500LL}},
    {"1 band, npt 200: two nodes per lane",
     {1, 200, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_pairs, 3, 2, 3, 1, 3, 25, 25u, 101u, 4208, 2, true, false, true, false, true, 40000LL}},
    {"2 bands, eigenvalues only, npt 97",
     {2, 97, 'r', 'E', 1, 5, 5, 1, 1, 1},
     {M::fused_lines, 11, 2, 2, 2, 1, 13, 13u, 49u, 3840, 2, true, false, true, false, true, 9409LL}},
    {"mirror, full layout, npt 149: 597 MB",
     {3, 149, 'r', 'F', 0, 5, 5, 1, 1, 1},
     {M::streamed, 24, 3, 3, 3, 1, 0, 2794u, 1u, 5456, 3, true, false, true, true, true, 11175LL}},
    {"mirror, full layout, npt 150: 605 MB, every plane",
     {3, 150, 'r', 'F', 0, 5, 5, 1, 1, 1},
     {M::streamed, 24, 3, 3, 3, 1, 0, 4096u, 1u, 5472, 3, true, false, false, true, true, 22500LL}},
    {"mirror, full layout, npt 150, ABZ_EVAL_MIRROR=2",
     {3, 150, 'r', 'F', 0, 5, 5, 1, 2, 1},
     {M::streamed, 24, 3, 3, 3, 1, 0, 2850u, 1u, 5472, 3, true, false, true, true, true, 11400LL}},
    {"non-temporal, npt 139: 267 MB, temporal stores",
     {3, 139, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_passwave, 24, 3, 3, 2, 2, 35, 35u, 70u, 7216, 3, true, false, true, false, true, 19321LL}},
    {"non-temporal, npt 140: 271 MB",
     {3, 140, 'r', 'C', 1, 5, 5, 1, 1, 1},
     {M::fused_passwave, 24, 3, 3, 2, 2, 35, 35u, 71u, 7232, 3, true, false, true, true, true, 19600LL}},
    {"block count, npt 141: 4971 quads, 8 per CU",
     {3, 141, 'r', 'F', 0, 5, 5, 1, 0, 1},
     {M::streamed, 24, 3, 3, 3, 1, 0, 2048u, 1u, 5328, 3, true, false, false, true, true, 19881LL}},
    {"block count, npt 142: 5041 quads, 16 per CU",
     {3, 142, 'r', 'F', 0, 5, 5, 1, 0, 1},
     {M::streamed, 24, 3, 3, 3, 1, 0, 4096u, 1u, 5344, 3, true, false, false, true, true, 20164LL}},
    {"block count, compact, npt 150, streamed: 24 per CU",
     {3, 150, 'r', 'C', 0, 5, 5, 1, 0, 1},
     {M::streamed, 24, 3, 3, 3, 1, 0, 5625u, 1u, 5472, 3, true, false, false, true, true, 22500LL}},
    {"eigenvectors (a velocity build), npt 150",
     {3, 150, 'r', 'U', 0, 5, 5, 1, 1, 1},
     {M::streamed, 45, 3, 3, 3, 1, 0, 4096u, 1u, 8160, 2, false, true, false, true, false, 22500LL}},
    {"general series, streamed, npt 64",
     {2, 64, 'g', 'F', 0, 5, 5, 1, 1, 1},
     {M::streamed, 20, 1, 1, 1, 1, 0, 1024u, 1u, 3584, 2, false, false, false, false, false, 4096LL}},
    {"fused LDS: 61440 + 16 npt bytes, npt 256 fits",
     {4, 256, 'g', 'F', 1, 15, 8, 1, 1, 1},
     {M::fused_lines, 240, 2, 2, 2, 2, 16, 16u, 256u, 65536, 2, false, false, false, true, false, 65536LL}},
    {"fused LDS: npt 257 does not",
     {4, 257, 'g', 'F', 1, 15, 8, 1, 1, 1},
     {M::unsupported, 240, 1, 1, 1, 5, 0, 0u, 1u, 0, 0, false, false, false, true, false, 66049LL}},
    {"fused, M2 16",
     {3, 64, 'r', 'C', 1, 5, 16, 1, 1, 1},
     {M::fused_lines, 24, 1, 1, 1, 1, 16, 16u, 33u, 10240, 3, true, false, true, false, true, 4096LL}},
    {"fused, M2 17 > ABZ_CONTRACT_GRID_MAXM",
     {3, 64, 'r', 'C', 1, 5, 17, 1, 1, 1},
     {M::unsupported, 24, 1, 1, 1, 1, 0, 0u, 1u, 0, 0, true, false, false, false, true, 4096LL}},
    {"fused with eigenvectors",
     {3, 64, 'r', 'U', 1, 5, 5, 1, 1, 1},
     {M::unsupported, 45, 1, 1, 1, 1, 0, 0u, 1u, 0, 0, true, false, false, false, false, 4096LL}},
    {"streamed, 256 numbers per line",
     {4, 100, 'g', 'F', 0, 16, 0, 1, 1, 1},
     {M::streamed, 256, 2, 2, 2, 1, 0, 2048u, 1u, 34368, 2, false, false, false, true, false, 10000LL}},
    {"scalar fallback, 272 numbers per line",
     {4, 100, 'g', 'F', 0, 17, 0, 1, 1, 1},
     {M::scalar, 272, 2, 2, 2, 1, 0, 2048u, 1u, 0, 0, false, false, false, true, false, 10000LL}},
    {"streamed LDS: 4224 + 16 npt bytes on packed sets, npt 3832 fits",
     {3, 3832, 'r', 'E', 0, 7, 0, 1, 1, 1},
     {M::streamed, 33, 3, 3, 3, 20, 0, 4096u, 1u, 65536, 3, true, false, false, true, true, 14684224LL}},
    {"streamed LDS: npt 3833 does not, with packed sets or without: scalar",
     {3, 3833, 'r', 'E', 0, 7, 0, 1, 1, 1},
     {M::scalar, 63, 3, 3, 3, 20, 0, 4096u, 1u, 0, 0, true, false, false, true, false, 14691889LL}},
    {"npt 65536: scalar",
     {1, 65536, 'r', 'E', 0, 1, 0, 1, 1, 1},
     {M::scalar, 1, 3, 3, 3, 342, 0, 4096u, 1u, 0, 0, true, false, false, true, false, 4294967296LL}},
    {"npt 65536, fused: unsupported",
     {1, 65536, 'r', 'E', 1, 1, 1, 1, 1, 1},
     {M::unsupported, 1, 3, 3, 3, 342, 0, 0u, 1u, 0, 0, true, false, false, true, false, 4294967296LL}},
};

static EvalRoute route_of(const Shape& p) {
    abz::EvalSwitches sw;
    sw.pairs = p.sw_pairs;
    sw.mirror = p.sw_mirror;
    sw.passwave = p.sw_passwave;
    sw.packed = 1;
    abz::EvalShape s;
    const int n = p.n, pitch = (p.npt + 15) / 16 * 16;  // rows of whole 128-B lines
    s.n = n;
    s.M = p.M;
    s.M2 = p.fused ? p.M2 : 0;
    s.npt = p.npt;
    s.nlines = (int64_t)p.npt * p.npt;
    s.herm = p.series != 'g';
    s.real_coef = p.series == 'r';
    s.velocity = p.out == 'U';
    s.fused = p.fused != 0;
    s.whole_grid3 = true;
    // one tile holds every plane of a line: H (full or the upper triangle), eigenvalues, velocities
    const bool compact = p.out == 'C' && s.herm;
    const int pH = p.out == 'E' ? 0 : (compact ? n * n : 2 * n * n), pE = n, pV = s.velocity ? 3 * n : 0;
    s.H.present = pH > 0;
    s.H.compact = compact;
    s.E.present = true;
    if (s.H.present) s.H.row = pitch, s.H.tile = (int64_t)(pH + pE + pV) * pitch;
    s.E.row = pitch, s.E.tile = (int64_t)(pH + pE + pV) * pitch;
    if (s.velocity) s.U.present = true, s.U.row = pitch, s.U.tile = (int64_t)2 * n * n * pitch;
    s.packed = s.herm && !s.velocity && abz::eval_packed_supported(n, p.M, p.npt, sw);
    return abz::eval_route(s, sw);
}

int main() {
    int bad = 0, ncases = 0;
    for (const Case& c : CASES) {
        const EvalRoute r = route_of(c.shape);
        const Expected& w = c.want;
        int miss = 0;
        auto chk = [&](const char* field, long long want, long long got) {
            if (want != got) {
                printf("%s: %s expected %lld, got %lld\n", c.what, field, want, got);
                ++miss;
            }
        };
        chk("mapping", (int)w.mapping, (int)r.mapping);
        chk("mnn", w.mnn, r.mnn);
        chk("kpl", w.kpl, r.kpl);
        chk("kp", w.kp, r.kp);
        chk("kt", w.kt, r.kt);
        chk("npass", w.npass, r.npass);
        chk("bpk", w.bpk, r.bpk);
        chk("grid_x", w.grid_x, r.grid_x);
        chk("grid_y", w.grid_y, r.grid_y);
        chk("lds", (long long)w.lds, (long long)r.lds);
        chk("occ", w.occ, r.occ);
        chk("herm", w.herm, r.herm);
        chk("vec", w.vec, r.vec);
        chk("mirror", w.mirror, r.mirror);
        chk("nt", w.nt, r.nt);
        chk("pk", w.pk, r.pk);
        chk("nlines", w.nlines, r.nlines);
        bad += miss != 0;
        ++ncases;
    }
    // the limits that rule_fill asks for before it builds the chain
    const abz::EvalSwitches on, off{1, 1, 1, 0};
    auto expect = [&](bool cond, const char* what) {
        if (!cond) {
            printf("%s\n", what);
            ++bad;
        }
    };
    expect(abz::eval_packed_supported(3, 5, 150, on), "packed sets: 3 bands, 5 coefficients");
    expect(!abz::eval_packed_supported(3, 5, 150, off), "packed sets: ABZ_EVAL_PACKED=0");
    expect(!abz::eval_packed_supported(3, 4, 150, on), "packed sets: an even coefficient count has no symmetric range");
    expect(!abz::eval_packed_supported(5, 5, 150, on), "packed sets: 5 bands");
    expect(abz::eval_fused_supported(3, 24, 16, 150) && !abz::eval_fused_supported(3, 24, 17, 150), "fused: M2 16 / 17");
    expect(abz::eval_fused_supported(4, 240, 8, 256) && !abz::eval_fused_supported(4, 240, 8, 257), "fused: LDS 65536 / 65552 bytes");
    expect(!abz::eval_fused_supported(4, 240, 8, 256, true), "fused pairs: four line sets per wave do not fit there");
    expect(abz::eval_kpl(150) == 3 && abz::eval_kpl(200) == 2 && abz::eval_kpl(64) == 1 && abz::eval_kpl(64, 2) == 2, "nodes per lane");
    if (bad) {
        printf("eval_route: %d of %d checks failed\n", bad, ncases + 8);
        return 1;
    }
    printf("eval_route: ok (%d cases)\n", ncases);
    return 0;
}
