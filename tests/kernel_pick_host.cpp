// pick() (csrc/kernel_pick.hpp) over every combination of two flags, a refusing list and a list with a fallback: the callable runs
// exactly once with the tags that equal the runtime values, or not at all.  Built by tests/test_kernel_pick_host.py with
// AddressSanitizer and UndefinedBehaviorSanitizer; needs no device and includes nothing of HIP.
#include <cstdio>
#include <type_traits>

#include "kernel_pick.hpp"

using isingmc::one_of;
using isingmc::or_last;
using isingmc::pick;

static int failures = 0, cases = 0;
#define CHECK(cond)                                                                                                    \
    do {                                                                                                               \
        if (!(cond) && failures++ < 20) std::printf("FAILED %s (line %d): a %d b %d rb %d lpq %d\n", #cond, __LINE__, a, b, rb, lpq); \
    } while (0)

int main()
{
    const int refusing[] = {8, 4, 2, 1, 0, 3, 16, -1, 2147483647};   // the list of one_of<8, 4, 2, 1> and values outside it
    const int fallback[] = {8, 4, 2, 0, 1, 3, 16, -8, -2147483647 - 1}; // the list of or_last<8, 4, 2> and values outside it
    for (int a = 0; a < 2; a++)
        for (int b = 0; b < 2; b++)
            for (int rb : refusing)
                for (int lpq : fallback) {
                    cases++;
                    int calls = 0;
                    bool got_a = false, got_b = false;
                    int got_rb = -99, got_lpq = -99;
                    const bool ok = pick(a != 0, b != 0, one_of<8, 4, 2, 1>{rb}, or_last<8, 4, 2>{lpq}, [&](auto A, auto B, auto RB, auto LPQ) {
                        static_assert(std::is_same_v<decltype(A), std::bool_constant<decltype(A)::value>>, "a flag is a bool_constant");
                        static_assert(std::is_same_v<decltype(B), std::bool_constant<decltype(B)::value>>, "a flag is a bool_constant");
                        static_assert(std::is_same_v<decltype(RB), std::integral_constant<int, decltype(RB)::value>>, "a list entry is an int constant");
                        static_assert(decltype(RB)::value == 8 || decltype(RB)::value == 4 || decltype(RB)::value == 2 || decltype(RB)::value == 1, "one_of: nothing but its list");
                        static_assert(decltype(LPQ)::value == 8 || decltype(LPQ)::value == 4 || decltype(LPQ)::value == 2, "or_last: nothing but its list");
                        calls++;
                        got_a = A.value, got_b = B.value, got_rb = RB.value, got_lpq = LPQ.value;
                    });
                    const bool listed = rb == 8 || rb == 4 || rb == 2 || rb == 1;
                    CHECK(ok == listed);
                    CHECK(calls == (listed ? 1 : 0));
                    if (listed) {
                        CHECK(got_a == (a != 0) && got_b == (b != 0));
                        CHECK(got_rb == rb);
                        CHECK(got_lpq == (lpq == 8 || lpq == 4 ? lpq : 2));
                    }
                }
    // the order of the choices is the order of the tags; one choice alone; a list of one entry; no choice at all
    {
        const int a = 1, b = 0, rb = 0, lpq = 0;
        int calls = 0;
        CHECK(pick(true, false, [&](auto A, auto B) { calls += A.value && !B.value; }) && calls == 1);
        CHECK(pick(or_last<7, 10>{7}, [&](auto N) { calls += N.value == 7; }) && calls == 2);
        CHECK(pick(or_last<7, 10>{8}, [&](auto N) { calls += N.value == 10; }) && calls == 3);
        CHECK(pick(or_last<5>{3}, one_of<5>{5}, [&](auto X, auto Y) { calls += X.value == 5 && Y.value == 5; }) && calls == 4);
        CHECK(!pick(one_of<5>{3}, true, [&](auto, auto) { calls += 100; }) && calls == 4);
        CHECK(!pick(true, one_of<3, 4, 5, 6>{7}, [&](auto, auto) { calls += 100; }) && calls == 4);
        CHECK(pick([&] { calls++; }) && calls == 5);
        cases += 7;
    }
    std::printf("kernel_pick_host: %d cases, %d failures\n", cases, failures);
    return failures ? 1 : 0;
}
