// The bit-sliced vertical counter of csrc/vertical_counter.hpp against per-bit counts, on the host (tests/test_moments_host.py
// builds this once plainly and once under AddressSanitizer + UndefinedBehaviorSanitizer).  For every K in 1 .. 16: exactly
// 2^K - 1 adds of random words (checked along the way) and of the all-ones word, which fills every plane.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "vertical_counter.hpp"

using namespace isingmc;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint32_t next_word() // xorshift64*
{
    rng_state ^= rng_state >> 12;
    rng_state ^= rng_state << 25;
    rng_state ^= rng_state >> 27;
    return uint32_t((rng_state * 0x2545F4914F6CDD1Dull) >> 32);
}

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d (K = %d): %s\n", __FILE__, __LINE__, K, #cond); \
            failures++;                                                          \
        }                                                                        \
    } while (0)

template <int K>
static void compare(const uint32_t (&planes)[K], const std::vector<uint32_t> &strided, const uint32_t (&naive)[32])
{
    uint32_t out[32];
    vc_expand(planes, out);
    for (int b = 0; b < 32; b++) {
        CHECK(out[b] == naive[b]);
        CHECK(vc_value(planes, b) == naive[b]);
    }
    for (int j = 0; j < K; j++) CHECK(strided[size_t(j) * 3 + 1] == planes[j]); // the strided form keeps the same planes
    for (int j = 0; j < K; j++) CHECK(strided[size_t(j) * 3] == 0 && strided[size_t(j) * 3 + 2] == 0); // ... and no other word
}

template <int K>
static void run()
{
    const uint32_t adds = (1u << K) - 1;
    for (int pattern = 0; pattern < 3; pattern++) { // random words, all ones, sparse words (one bit each)
        uint32_t planes[K] = {}, naive[32] = {};
        std::vector<uint32_t> strided(3 * size_t(K), 0u); // planes 3 words apart, the middle word of each is the counter's
        for (uint32_t n = 0; n < adds; n++) {
            const uint32_t w = pattern == 0 ? next_word() : pattern == 1 ? ~0u : 1u << (next_word() & 31);
            vc_add(planes, w);
            vc_add_strided(strided.data() + 1, 3, K, w);
            for (int b = 0; b < 32; b++) naive[b] += (w >> b) & 1u;
            if (n % 97 == 0 || n + 1 == adds) compare(planes, strided, naive);
        }
        if (pattern == 1)
            for (int j = 0; j < K; j++) CHECK(planes[j] == ~0u); // 2^K - 1 in every counter: all planes full
    }
}

template <int K>
static void run_all()
{
    run<K>();
    if constexpr (K > 1) run_all<K - 1>();
}

int main()
{
    run_all<16>();
    if (failures) {
        std::printf("vertical_counter_host: %d check(s) failed\n", failures);
        return 1;
    }
    std::printf("vertical_counter_host: ok\n");
    return 0;
}
