// Stand-alone check of abz::DevBuf (csrc/dev_buf.h) by a plain host compiler: ownership, moves, views, the growth rule and
// "no block survives an early exit".  dev_alloc / dev_free are supplied here: malloc / free with a table of live blocks, a
// counter that makes the N-th allocation fail, and a free of an unknown (or already freed) pointer counted, not performed.
// Exit status 0 only if every check held, the table is empty at the end and no bad free was seen.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <stdexcept>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../autobzcore.jl_amd/csrc/dev_buf.h"

namespace {
std::map<void*, size_t> g_live;       // block -> bytes asked for
std::vector<size_t> g_requests;       // every request, failed ones included
int g_allocs = 0, g_fail_at = 0, g_fail_count = 0;  // requests g_fail_at ... g_fail_at + g_fail_count - 1 from now fail
int g_bad_frees = 0, g_frees = 0, g_failed = 0;

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::fprintf(stderr, "line %d: %s is false\n", __LINE__, #cond); \
            g_failed += 1;                                                 \
        }                                                                  \
    } while (0)

void fail_nth(int n, int count = 1) {  // n = 0: none
    g_allocs = 0;
    g_fail_at = n;
    g_fail_count = n ? count : 0;
}
}  // namespace

namespace abz {
int dev_alloc(void** out, size_t bytes, size_t* cap_out) {
    g_requests.push_back(bytes);
    g_allocs += 1;
    if (g_allocs >= g_fail_at && g_allocs < g_fail_at + g_fail_count) {
        *out = nullptr;  // (cap_out is left alone, like the library's allocator on failure)
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
    if (it == g_live.end() || it->second != cap) {  // unknown, freed before, or with another size than it was handed out
        g_bad_frees += 1;
        return;
    }
    g_live.erase(it);
    g_frees += 1;
    std::free(p);
}
}  // namespace abz

using abz::DevBuf;

static_assert(!std::is_copy_constructible<DevBuf>::value && !std::is_copy_assignable<DevBuf>::value, "DevBuf is move-only");
static_assert(std::is_nothrow_move_constructible<DevBuf>::value && std::is_nothrow_move_assignable<DevBuf>::value, "moves are noexcept");

// shaped like PlanDev / RulePlan of api.cpp
struct PlanLike {
    DevBuf gi[4], xs[4], parent[4], phg[4];
    DevBuf runs, arena;
};
struct RuleLike {
    PlanLike pd;
    DevBuf tab, tmpU, tmpD, fam[2], tri;
};

static void test_reserve_growth() {
    {
        DevBuf b;
        g_requests.clear();
        CHECK(b.reserve(1000) == 0);
        CHECK(g_requests.size() == 1 && g_requests[0] == 1000 + 250 + 256);
        CHECK(b.p && b.cap == 1506 && !b.view);
        void* const p0 = b.p;
        CHECK(b.reserve(1) == 0 && b.reserve(1506) == 0);  // bytes <= cap: nothing happens
        CHECK(b.p == p0 && g_requests.size() == 1);
        CHECK(b.reserve(1507) == 0);  // one more byte: a new block, the old one freed first
        CHECK(g_requests.size() == 2 && g_requests[1] == 1507 + 376 + 256 && g_live.size() == 1);
        // the larger request fails: the exact size is asked for
        g_requests.clear();
        fail_nth(1);
        CHECK(b.reserve(4000) == 0);
        CHECK(g_requests.size() == 2 && g_requests[0] == 4000 + 1000 + 256 && g_requests[1] == 4000 && b.cap == 4000);
        // both fail: the allocator's status, the buffer empty (the old block was released first), nothing live
        g_requests.clear();
        fail_nth(1, 2);
        CHECK(b.reserve(8000) == -2);
        CHECK(g_requests.size() == 2 && g_requests[1] == 8000 && !b.p && b.cap == 0 && g_live.empty());
        fail_nth(0);
        CHECK(b.reserve(8) == 0 && b.cap == 8 + 2 + 256);  // and it serves again
    }
    CHECK(g_live.empty());
}

static void test_alloc_exact() {
    {
        DevBuf b;
        g_requests.clear();
        CHECK(b.alloc(346) == 0);
        CHECK(g_requests.size() == 1 && g_requests[0] == 346 && b.cap == 346);
        CHECK(b.alloc(100) == 0);  // always a fresh block, the old one released first
        CHECK(g_requests.size() == 2 && g_requests[1] == 100 && b.cap == 100 && g_live.size() == 1);
        fail_nth(1);
        CHECK(b.alloc(50) != 0);  // a failure leaves the buffer empty (the old block is gone: it was released first)
        CHECK(!b.p && b.cap == 0 && !b.view && g_live.empty());
        fail_nth(0);
    }
    CHECK(g_live.empty());
}

static void test_moves() {
    {
        DevBuf a;
        CHECK(a.alloc(10) == 0);
        void* const pa = a.p;
        DevBuf b(std::move(a));  // move construction: the source is empty
        CHECK(b.p == pa && b.cap == 10 && !a.p && a.cap == 0 && !a.view);
        DevBuf c;
        CHECK(c.alloc(20) == 0);
        const int frees = g_frees;
        c = std::move(b);  // into a non-empty target: what it held is released
        CHECK(g_frees == frees + 1 && c.p == pa && c.cap == 10 && !b.p && g_live.size() == 1);
        DevBuf& self = c;
        c = std::move(self);  // self-move: nothing happens
        CHECK(c.p == pa && c.cap == 10 && g_live.size() == 1);
        c = DevBuf();  // dropping by assigning an empty buffer
        CHECK(!c.p && g_live.empty());
        // a view moves as a view
        int x = 0;
        DevBuf v = DevBuf::view_of(&x);
        DevBuf w(std::move(v));
        CHECK(w.view && w.p == &x && !v.view && !v.p);
    }
    CHECK(g_live.empty());
}

static void test_views() {
    char arena[64];
    const int frees = g_frees;
    {
        DevBuf v = DevBuf::view_of(arena + 8);
        CHECK(v.view && v.p == arena + 8 && v.cap == 0 && v.as<char>() == arena + 8);
    }  // forgotten, not freed
    CHECK(g_frees == frees && g_bad_frees == 0);
    {
        DevBuf v = DevBuf::view_of(arena);
        v.release();
        CHECK(!v.p && !v.view && g_frees == frees && g_bad_frees == 0);
        v = DevBuf::view_of(arena);
        CHECK(v.reserve(0) == 0);  // reserve on a view allocates fresh, whatever the size
        CHECK(!v.view && v.p != arena && v.cap == 256 && g_live.size() == 1);
        DevBuf o;
        CHECK(o.alloc(32) == 0);
        o = DevBuf::view_of(arena);  // a view into an owner: the block goes, the view stays a view
        CHECK(o.view && g_live.size() == 1);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
}

static void test_containers() {
    {
        DevBuf arr[8];
        for (int i = 0; i < 8; i += 2) CHECK(arr[i].reserve(100 + i) == 0);
        CHECK(g_live.size() == 4);
    }
    CHECK(g_live.empty());
    {  // what the context's phase cache does: emplace_back of an empty buffer, filled in place, the vector growing
        std::vector<std::pair<int, DevBuf>> cache;
        for (int npt = 1; npt <= 40; ++npt) {
            cache.emplace_back(npt, DevBuf());
            DevBuf& c = cache.back().second;
            if (npt % 7 == 0) {
                cache.pop_back();  // (an entry that could not be filled)
                continue;
            }
            CHECK(c.reserve(16 * (size_t)npt) == 0);
        }
        CHECK(g_live.size() == cache.size() && cache.size() == 35);
        for (auto& e : cache) CHECK(e.second.p && g_live.count(e.second.p) == 1);
        cache.erase(cache.begin());
        CHECK(g_live.size() == 34);
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
    {
        RuleLike* r = new RuleLike();
        CHECK(r->pd.arena.reserve(1000) == 0);
        for (int L = 0; L < 3; ++L) {  // views into the arena, as in a device-built symmetric rule
            r->pd.gi[L] = DevBuf::view_of(r->pd.arena.as<char>() + 10 * L);
            r->pd.parent[L] = DevBuf::view_of(r->pd.arena.as<char>() + 100 + 10 * L);
        }
        CHECK(r->pd.phg[1].reserve(64) == 0 && r->tab.reserve(64) == 0 && r->tmpU.reserve(64) == 0 && r->fam[1].reserve(8) == 0);
        r->tmpU.release();
        CHECK(g_live.size() == 4);
        delete r;
    }
    CHECK(g_live.empty() && g_bad_frees == 0);
}

static int five_buffers(bool throw_at_end) {
    DevBuf flag, counts, offs, didx, dw;
    int rc;
    if ((rc = flag.reserve(400))) return rc;
    if ((rc = counts.reserve(40))) return rc;
    if ((rc = offs.alloc(80))) return rc;
    if ((rc = didx.reserve(1200)) || (rc = dw.alloc(800))) return rc;
    if (throw_at_end) throw std::runtime_error("left early");
    return 0;
}

static void test_early_exits() {
    bool caught = false;
    try {
        (void)five_buffers(true);
    } catch (const std::runtime_error&) {
        caught = true;
    }
    CHECK(caught && g_live.empty());
    // the N-th allocation fails.  A reserve asks twice before it gives up, so five buffers are up to eight requests; every N is
    // walked, those that only trigger a fallback included.
    int refusals = 0;
    for (int n = 1; n <= 9; ++n) {
        fail_nth(n);
        const int rc = five_buffers(false);
        fail_nth(0);
        refusals += rc != 0;
        CHECK(g_live.empty());
    }
    CHECK(refusals == 2);  // the two exact-size allocations; a failed first request of a reserve falls back
    // ... and with the request after it failing as well, so that every one of the five refuses in turn
    refusals = 0;
    for (int n = 1; n <= 5; ++n) {
        fail_nth(n, 2);
        const int rc = five_buffers(false);
        fail_nth(0);
        refusals += rc != 0;
        CHECK(g_live.empty());
    }
    CHECK(refusals == 5);
}

int main() {
    test_reserve_growth();
    test_alloc_exact();
    test_moves();
    test_views();
    test_containers();
    test_early_exits();
    if (!g_live.empty()) std::fprintf(stderr, "%zu blocks are still live\n", g_live.size());
    if (g_bad_frees) std::fprintf(stderr, "%d frees of unknown or already freed blocks\n", g_bad_frees);
    const bool ok = g_failed == 0 && g_live.empty() && g_bad_frees == 0;
    std::printf("devbuf: %s (%d frees, %d failed checks)\n", ok ? "ok" : "FAILED", g_frees, g_failed);
    return ok ? 0 : 1;
}
