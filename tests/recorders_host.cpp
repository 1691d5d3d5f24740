// Periodic (csrc/host_logic.hpp) against a brute-force walk over timesteps: recorders_host <cases> <seed>.  Built by
// tests/test_recorders_host.py with AddressSanitizer and UndefinedBehaviorSanitizer; needs no device.
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <vector>

#include "host_logic.hpp"

using isingmc::Periodic;

static int failures = 0;
#define CHECK(cond)                                                                                                             \
    do {                                                                                                                        \
        if (!(cond) && failures++ < 20)                                                                                         \
            std::printf("FAILED %s (line %d): t0 %" PRIu64 " every %zu t %" PRIu64 " n %" PRIu64 "\n", #cond, __LINE__, t0, every, t, n); \
    } while (0)

// the sample points the step loop takes when it walks (t, t + n] in stretches, as run_steps_impl does
static std::vector<uint64_t> walk(Periodic &p, uint64_t t, uint64_t n)
{
    std::vector<uint64_t> taken;
    const uint64_t end = t + n;
    while (t < end) {
        t += std::min<uint64_t>(end - t, p.stretch(t));
        if (p.due(t)) {
            taken.push_back(t);
            p.last_t = t;
        }
    }
    return taken;
}

int main(int argc, char **argv)
{
    const int cases = argc > 1 ? std::atoi(argv[1]) : 400;
    std::mt19937_64 rng(argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 1);
    const uint64_t top = std::numeric_limits<uint64_t>::max();
    for (int c = 0; c < cases; c++) {
        const size_t every = c % 5 == 0 ? 1 : size_t(1 + rng() % (c % 3 ? 7 : 40));
        const uint64_t n = rng() % 60;
        uint64_t t0 = c % 4 == 0 ? 0 : rng() % 1000, t = t0 + rng() % 200;
        if (c % 7 == 3) { // the last timesteps a 64-bit clock can hold
            t = top - 64 - rng() % 3; // (t + n and the next sample point stay below 2^64)
            t0 = c % 2 ? t - rng() % 50 : rng() % 1000;
        }
        Periodic p;
        p.every = every;
        p.restart(t0);
        std::vector<uint64_t> brute; // u in (t, t + n] with (u - t0) % every == 0
        for (uint64_t u = t + 1; u - t <= n && u != 0; u++)
            if ((u - t0) % every == 0) brute.push_back(u);
        CHECK(p.points(t, n) == brute.size());
        // stretch lands exactly on the next sample point
        uint64_t next = t + 1;
        while ((next - t0) % every != 0) next++;
        CHECK(t + p.stretch(t) == next);
        CHECK(!p.due(t) || (t - t0) % every == 0);
        // a call walked in stretches takes exactly those samples
        const std::vector<uint64_t> taken = walk(p, t, n);
        CHECK(taken == brute);
        CHECK(p.last_t == (brute.empty() ? 0 : brute.back()));
        // the repeat of the call after its first attempt got as far as the k-th sample takes the rest, and nothing twice
        if (!brute.empty()) {
            const size_t k = rng() % brute.size();
            p.last_t = brute[k];
            p.replay_since(t);
            CHECK(p.replay_to == brute[k]);
            const std::vector<uint64_t> again = walk(p, t, n);
            CHECK(again == std::vector<uint64_t>(brute.begin() + k + 1, brute.end()));
            p.replay_to = 0;
        }
        // a first attempt that took no sample of this call (the last one lies before it) is repeated in full
        p.last_t = t;
        p.replay_since(t);
        CHECK(p.replay_to == 0);
        CHECK(walk(p, t, n) == brute);
        // off: nothing is ever due, no stretch ends, and the replay guard stays clear
        Periodic off;
        off.restart(t0);
        off.last_t = t + 1;
        off.replay_since(t);
        CHECK(off.replay_to == 0 && off.stretch(t) == std::numeric_limits<size_t>::max());
        for (uint64_t u = t; u - t <= n && (u != 0 || u == t); u++) CHECK(!off.due(u));
    }
    std::printf("recorders_host: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
