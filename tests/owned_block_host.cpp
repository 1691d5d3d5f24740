// Stand-alone check of csrc/owned_block.hpp with a counting free function in place of the block caches (built with ASan + UBSan
// by tests/test_owned_block_host.py).  The free function only counts, so that no address comes round twice; main deletes every
// block at the end: one that was never handed back is then the leak checker's finding as well.
#include <cstdio>
#include <map>
#include <type_traits>
#include <utility>
#include <vector>

#include "owned_block.hpp"

static std::map<void *, int> g_freed; // block -> times freed
static int g_frees = 0;
static void counting_free(void *p)
{
    g_freed[p]++;
    g_frees++;
}
using Block = OwnedBlock<int, counting_free>;
static_assert(!std::is_copy_constructible<Block>::value && !std::is_copy_assignable<Block>::value, "move-only");
static_assert(sizeof(Block) == sizeof(int *), "a handle is its pointer");

static int g_failures = 0;
#define CHECK(cond)                                                                    \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            std::printf("owned_block_host: line %d: %s\n", __LINE__, #cond);           \
            g_failures++;                                                              \
        }                                                                              \
    } while (0)

static int *fresh(int tag)
{
    int *p = new int[4];
    p[0] = tag;
    return p;
}

// what dev_alloc does: the new block into a temporary, moved in on success only
static bool alloc_into(Block &out, int tag, bool succeed)
{
    if (!succeed) return false;
    out = Block(fresh(tag));
    return true;
}

int main()
{
    { // an empty handle frees nothing, on destruction or on reset
        Block e;
        CHECK(e.get() == nullptr && !e);
        e.reset();
    }
    CHECK(g_frees == 0);

    int *a = fresh(1);
    { // destruction frees once; the conversion reads as the raw pointer does
        Block b(a);
        CHECK(b.get() == a && b == a && b + 1 == a + 1 && b[0] == 1 && *b == 1);
        int *raw = b;
        CHECK(raw == a);
        CHECK(g_frees == 0);
    }
    CHECK(g_frees == 1 && g_freed[a] == 1);

    int *b1 = fresh(2);
    { // move construction leaves the source empty: one free for the two handles
        Block src(b1);
        Block dst(std::move(src));
        CHECK(src.get() == nullptr && dst.get() == b1);
        CHECK(g_frees == 1);
    }
    CHECK(g_frees == 2 && g_freed[b1] == 1);

    int *c1 = fresh(3), *c2 = fresh(4);
    { // move assignment frees the target's old block exactly once, at once, and empties the source
        Block src(c1), dst(c2);
        dst = std::move(src);
        CHECK(g_frees == 3 && g_freed[c2] == 1 && g_freed.count(c1) == 0);
        CHECK(src.get() == nullptr && dst.get() == c1);
        Block &self = dst;
        dst = std::move(self); // onto itself: nothing happens
        CHECK(dst.get() == c1 && g_frees == 3);
    }
    CHECK(g_frees == 4 && g_freed[c1] == 1 && g_freed[c2] == 1);

    { // an attach that failed half way left blocks in the fields: the next attach assigns over them and the old ones go back
        Block ladder, perm;
        CHECK(alloc_into(ladder, 5, true));
        CHECK(!alloc_into(perm, 6, false)); // the failure: `perm` stays empty, `ladder` keeps its block
        int *stale = ladder.get();
        CHECK(stale && !perm && g_frees == 4);
        CHECK(alloc_into(ladder, 7, true)); // the second attach
        CHECK(g_frees == 5 && g_freed[stale] == 1 && ladder.get() != nullptr && ladder[0] == 7);
        CHECK(alloc_into(perm, 8, true));
        CHECK(g_frees == 5);
        CHECK(!alloc_into(ladder, 9, false)); // a failed allocation keeps what the handle held
        CHECK(g_frees == 5 && ladder[0] == 7);
    }
    CHECK(g_frees == 7);

    int *d = fresh(10);
    { // reset() twice frees once
        Block b(d);
        b.reset();
        CHECK(g_frees == 8 && b.get() == nullptr);
        b.reset();
        CHECK(g_frees == 8);
    }
    CHECK(g_frees == 8 && g_freed[d] == 1);

    int *s1 = fresh(11), *s2 = fresh(12);
    { // swap frees nothing, also with an empty handle
        Block x(s1), y(s2), e;
        x.swap(y);
        CHECK(x.get() == s2 && y.get() == s1 && g_frees == 8);
        x.swap(e);
        CHECK(x.get() == nullptr && e.get() == s2 && g_frees == 8);
    }
    CHECK(g_frees == 10 && g_freed[s1] == 1 && g_freed[s2] == 1);

    std::vector<int *> raw;
    { // a vector of handles frees each element once, across its reallocations
        std::vector<Block> v;
        for (int i = 0; i < 100; i++) {
            raw.push_back(fresh(100 + i));
            v.push_back(Block(raw.back()));
        }
        CHECK(g_frees == 10);
        for (int i = 0; i < 100; i++) CHECK(v[i].get() == raw[i] && v[i][0] == 100 + i);
        v.erase(v.begin() + 10); // the elements behind move down one place
        CHECK(g_frees == 11 && g_freed[raw[10]] == 1);
    }
    CHECK(g_frees == 110);
    for (int *p : raw) CHECK(g_freed[p] == 1);
    for (const auto &kv : g_freed) {
        CHECK(kv.second == 1);
        delete[] static_cast<int *>(kv.first);
    }

    if (g_failures) return 1;
    std::printf("owned_block_host: ok, %d blocks freed once each\n", g_frees);
    return 0;
}
