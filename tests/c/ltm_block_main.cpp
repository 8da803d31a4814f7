// Stand-alone check of abz::LtmBlock (csrc/ltm_block.h) by a plain host compiler: the view and the byte count of a block tiled
// like eigenvalue planes with padded rows, the views of its sets, and the "complete before it replaces the resident one"
// discipline -- a failed allocation leaves the local block empty and the resident one untouched, a move-in frees the old
// block exactly once, dropping twice is harmless.  dev_alloc / dev_free are supplied here as in devbuf_main.cpp: malloc / free
// with a table of live blocks, an allocation that fails on demand, a bad free counted and not performed.
// Exit status 0 only if every check held, the table is empty at the end and no bad free was seen.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <type_traits>
#include <utility>

#include "../../autobzcore.jl_amd/csrc/ltm_block.h"

namespace {
std::map<void*, size_t> g_live;  // block -> bytes asked for
size_t g_last_request = 0;
bool g_fail_next = false;
int g_bad_frees = 0, g_frees = 0, g_failed = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            g_failed += 1;                                                 \
        }                                                                  \
    } while (0)
}  // namespace

namespace abz {
int dev_alloc(void** out, size_t bytes, size_t* cap_out) {
    g_last_request = bytes;
    if (g_fail_next) {
        g_fail_next = false;
        *out = nullptr;
        return -2;
    }
    *out = std::malloc(bytes ? bytes : 1);
    if (!*out) return -2;
    g_live[*out] = bytes;
    if (cap_out) *cap_out = bytes;
    return 0;
}
void dev_free(void* p, size_t cap) {
    if (!p) return;
    auto it = g_live.find(p);
    if (it == g_live.end() || it->second != cap) {
        g_bad_frees += 1;
        return;
    }
    g_live.erase(it);
    g_frees += 1;
    std::free(p);
}
}  // namespace abz

using abz::LtmBlock;
using abz::PlaneView;

static_assert(!std::is_copy_constructible<LtmBlock>::value && !std::is_copy_assignable<LtmBlock>::value, "LtmBlock is move-only");
static_assert(std::is_nothrow_move_constructible<LtmBlock>::value && std::is_nothrow_move_assignable<LtmBlock>::value, "moves are noexcept");

// the eigenvalue planes of a rule of 3 grid lines of 5 nodes in rows padded to 16: 4 planes per tile, a compact marker that the
// block must not inherit
static PlaneView planes_like(double* base) {
    PlaneView E;
    E.base = base;
    E.tile = 4 * 16;
    E.pitch = 16;
    E.line_len = 5;
    E.row = 16;
    E.compact = 4;
    return E;
}

static void test_tiling() {
    double eig[1];
    const PlaneView E = planes_like(eig);
    const int64_t ntiles = 3;
    const int per = 2, sets = 3;  // 2 planes x 3 sets
    {
        LtmBlock b;
        CHECK(!b.buf.p && b.sets == 0 && b.bytes(ntiles, per) == 0);
        CHECK(LtmBlock::bytes(E, ntiles, per * sets) == sizeof(double) * 3 * 6 * 16);  // padded rows, not line_len
        CHECK(b.alloc(E, ntiles, per, sets) == 0);
        CHECK(g_last_request == sizeof(double) * 3 * 6 * 16 && b.buf.cap == g_last_request);
        CHECK(b.bytes(ntiles, per) == g_last_request && b.sets == 3);
        CHECK(b.view.base == b.buf.as<double>() && b.view.base != eig);
        CHECK(b.view.tile == 6 * 16 && b.view.pitch == 16 && b.view.line_len == 5 && b.view.row == 16 && b.view.compact == 0);
        for (int i = 0; i < sets; ++i) {
            const PlaneView v = b.set_view(i, per);
            CHECK(v.base == b.view.base + (int64_t)i * per * 16);
            CHECK(v.tile == b.view.tile && v.pitch == 16 && v.line_len == 5 && v.row == 16 && v.compact == 0);
        }
        // the last element of the last set's last plane in the last tile is the block's last padded row
        const PlaneView last = b.set_view(sets - 1, per);
        const int64_t k = 3 * 5 - 1;  // node 14: tile 2, column 4
        const double* e = last.base + (k / last.line_len) * last.tile + (int64_t)(per - 1) * last.pitch + k % last.line_len;
        CHECK(e - b.view.base == 3 * 6 * 16 - 16 + 4);
        CHECK((size_t)(e - b.view.base) < b.bytes(ntiles, per) / sizeof(double));
        // a second alloc: a fresh block of the new shape, the old one released first
        const int frees = g_frees;
        CHECK(b.alloc(E, ntiles, 4, 1) == 0);
        CHECK(g_frees == frees + 1 && g_live.size() == 1 && b.sets == 1 && b.view.tile == 4 * 16 && b.bytes(ntiles, 4) == sizeof(double) * 3 * 4 * 16);
    }
    CHECK(g_live.empty());
}

// what every entry point that replaces a resident block does: build into a local block, move it in when it is complete
static int replace(LtmBlock& resident, const PlaneView& E, int per, int sets) {
    LtmBlock block;
    const int rc = block.alloc(E, 3, per, sets);
    if (rc) {
        CHECK(!block.buf.p && block.buf.cap == 0 && block.sets == 0 && !block.view.base && block.bytes(3, per) == 0);
        return rc;
    }
    resident = std::move(block);
    CHECK(!block.buf.p && block.bytes(3, per) == 0);  // what was moved from owns nothing
    return 0;
}

static void test_replace_and_drop() {
    double eig[1];
    const PlaneView E = planes_like(eig);
    {
        LtmBlock resident;
        CHECK(replace(resident, E, 2, 3) == 0);
        void* const p0 = resident.buf.p;
        const PlaneView v0 = resident.view;
        CHECK(p0 && g_live.size() == 1);
        // a failed allocation: the resident block is as it was
        int frees = g_frees;
        g_fail_next = true;
        CHECK(replace(resident, E, 2, 5) != 0);
        CHECK(resident.buf.p == p0 && resident.sets == 3 && resident.view.base == v0.base && resident.view.tile == v0.tile);
        CHECK(g_frees == frees && g_live.size() == 1 && g_live.count(p0) == 1);
        // a move-in frees the old block exactly once
        CHECK(replace(resident, E, 2, 5) == 0);
        CHECK(g_frees == frees + 1 && g_live.size() == 1 && g_live.count(p0) == 0);
        CHECK(resident.buf.p != nullptr && resident.sets == 5 && resident.view.tile == 10 * 16 && resident.view.base == resident.buf.as<double>());
        // moving an empty block in drops the resident one (a pair rule refilled without operators)
        frees = g_frees;
        resident = LtmBlock();
        CHECK(g_frees == frees + 1 && !resident.buf.p && resident.sets == 0 && !resident.view.base && g_live.empty());
        // drop() twice is harmless, on a full and on an empty block
        CHECK(replace(resident, E, 1, 1) == 0);
        frees = g_frees;
        resident.drop();
        CHECK(g_frees == frees + 1 && !resident.buf.p && resident.sets == 0 && !resident.view.base && resident.view.row == 0);
        resident.drop();
        CHECK(g_frees == frees + 1 && g_bad_frees == 0 && g_live.empty());
        // a failed alloc on a full block leaves it empty (the old block is released first, as DevBuf::alloc does)
        CHECK(resident.alloc(E, 3, 2, 2) == 0);
        g_fail_next = true;
        CHECK(resident.alloc(E, 3, 2, 2) != 0);
        CHECK(!resident.buf.p && resident.sets == 0 && !resident.view.base && g_live.empty());
        CHECK(resident.alloc(E, 3, 2, 2) == 0);  // and it serves again; the destructor lets this one go
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
}

int main() {
    test_tiling();
    test_replace_and_drop();
    if (!g_live.empty()) std::fprintf(stderr, "%zu blocks are still live\n", g_live.size());
    if (g_bad_frees) std::fprintf(stderr, "%d frees of unknown or already freed blocks\n", g_bad_frees);
    const bool ok = g_failed == 0 && g_live.empty() && g_bad_frees == 0;
    std::printf("ltm_block: %s (%d frees, %d failed checks)\n", ok ? "ok" : "FAILED", g_frees, g_failed);
    return ok ? 0 : 1;
}
