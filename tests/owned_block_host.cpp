// Stand-alone check of csrc/owned_block.hpp with counting free functions in place of the block caches and of the stream and
// event pools (built with ASan + UBSan by tests/test_owned_block_host.py).  The free function only counts, so that no address comes round twice; main deletes every
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

// The pooled handles: this program is the pool.  A stream or an event is an opaque value here, the address of a tag that is
// never read through; every release is counted per value and, for events, per kind.
static std::map<const void *, int> g_released; // handle value -> times released
static int g_stream_releases = 0, g_event_releases[2] = {0, 0}; // events: [timing disabled?]
void pooled_stream_destroy(ihipStream_t *st)
{
    g_released[st]++;
    g_stream_releases++;
}
void pooled_event_destroy(ihipEvent_t *ev, bool disable_timing)
{
    g_released[ev]++;
    g_event_releases[disable_timing ? 1 : 0]++;
}
static char g_tags[16];
static ihipStream_t *stream_value(int i) { return reinterpret_cast<ihipStream_t *>(&g_tags[i]); }
static ihipEvent_t *event_value(int i) { return reinterpret_cast<ihipEvent_t *>(&g_tags[i]); }
static_assert(!std::is_copy_constructible<PooledStream>::value && !std::is_copy_assignable<PooledStream>::value, "move-only");
static_assert(!std::is_copy_constructible<PooledEvent>::value && !std::is_copy_assignable<TimedEvent>::value, "move-only");
static_assert(!std::is_same<PooledEvent, TimedEvent>::value && !std::is_convertible<PooledEvent, TimedEvent>::value &&
                  !std::is_assignable<TimedEvent &, PooledEvent>::value, "an event's kind is part of its type");
static_assert(sizeof(PooledStream) == sizeof(void *) && sizeof(TimedEvent) == sizeof(void *), "a handle is its value");

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

static void pooled_handles()
{
    { // a default-constructed handle releases nothing, on destruction, on reset or when it is moved from
        PooledStream s;
        PooledEvent e;
        TimedEvent t;
        CHECK(s.get() == nullptr && !s && !e && !t);
        s.reset();
        PooledStream s2(std::move(s));
        PooledEvent arr[2]; // as the members ev[2] of a container
        CHECK(!arr[0] && !arr[1] && !s2);
    }
    CHECK(g_stream_releases == 0 && g_event_releases[0] == 0 && g_event_releases[1] == 0);

    { // destruction releases once; the conversion reads as the raw handle does
        PooledStream s(stream_value(0));
        ihipStream_t *raw = s;
        CHECK(raw == stream_value(0) && s.get() == raw && s == stream_value(0) && s);
        CHECK(g_stream_releases == 0);
    }
    CHECK(g_stream_releases == 1 && g_released[stream_value(0)] == 1);

    { // move construction: one release for the two handles
        PooledStream src(stream_value(1));
        PooledStream dst(std::move(src));
        CHECK(!src && dst.get() == stream_value(1) && g_stream_releases == 1);
    }
    CHECK(g_stream_releases == 2 && g_released[stream_value(1)] == 1);

    { // move assignment over a held value releases that value exactly once, at once, and empties the source
        PooledStream src(stream_value(2)), dst(stream_value(3));
        dst = std::move(src);
        CHECK(g_stream_releases == 3 && g_released[stream_value(3)] == 1 && g_released.count(stream_value(2)) == 0);
        CHECK(!src && dst.get() == stream_value(2));
        PooledStream &self = dst;
        dst = std::move(self); // onto itself: nothing happens
        CHECK(dst.get() == stream_value(2) && g_stream_releases == 3);
    }
    CHECK(g_stream_releases == 4 && g_released[stream_value(2)] == 1 && g_released[stream_value(3)] == 1);

    { // reset() twice releases once
        PooledStream s(stream_value(4));
        s.reset();
        CHECK(g_stream_releases == 5 && !s);
        s.reset();
        CHECK(g_stream_releases == 5);
    }
    CHECK(g_stream_releases == 5 && g_released[stream_value(4)] == 1);

    { // what the creation helpers do: the new value into a temporary, assigned over whatever the handle held
        PooledEvent e;
        e = PooledEvent(event_value(5));
        CHECK(g_event_releases[1] == 0);
        e = PooledEvent(event_value(6));
        CHECK(g_event_releases[1] == 1 && g_released[event_value(5)] == 1 && e.get() == event_value(6));
    }
    CHECK(g_event_releases[1] == 2 && g_event_releases[0] == 0 && g_released[event_value(6)] == 1);

    { // each kind of event reaches its own release: no timing event ends up in the other pool
        TimedEvent t(event_value(7));
        CHECK(g_event_releases[0] == 0);
    }
    CHECK(g_event_releases[0] == 1 && g_event_releases[1] == 2 && g_released[event_value(7)] == 1);
    {
        PooledEvent e(event_value(8));
        TimedEvent t0(event_value(9)), t1(event_value(10));
    }
    CHECK(g_event_releases[0] == 3 && g_event_releases[1] == 3 && g_stream_releases == 5);

    { // the lanes of a container: a vector of handles releases each element once, across its reallocations
        std::vector<PooledStream> lanes;
        for (int i = 11; i < 16; i++) {
            PooledStream st(stream_value(i));
            lanes.push_back(std::move(st));
        }
        CHECK(g_stream_releases == 5);
        int seen = 0;
        for (ihipStream_t *st : lanes) seen += st == stream_value(11 + seen) ? 1 : 0; // iterating by value copies no handle
        CHECK(seen == 5 && g_stream_releases == 5);
    }
    CHECK(g_stream_releases == 10);
    for (const auto &kv : g_released) CHECK(kv.second == 1);
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

    pooled_handles();

    if (g_failures) return 1;
    std::printf("owned_block_host: ok, %d blocks freed once each\n", g_frees);
    return 0;
}
