// Host check of csrc/scan_dispatch.h (tests/test_scan_dispatch_cpu.py builds it with the address and undefined-behaviour
// sanitizers): which constant by_code_size hands over for every code size, what the run-time form accepts, and the arity
// with_mask calls with.  Includes nothing else of the library; exit status 0 = every check held.
#include "scan_dispatch.h"

#include <cstdio>

using namespace ivfhnsw_gpu_impl;

static int failures = 0;
#define CHECK(cond, ...)             \
    do {                             \
        if (!(cond)) {               \
            failures++;              \
            printf("FAIL: " __VA_ARGS__); \
            printf("\n");            \
        }                            \
    } while (0)

int main()
{
    for (int M = 0; M <= 132; M++) {
        int calls = 0;
        const int got = by_code_size<4, 8, 16, 32>(M, [&](auto cs) {
            calls++;
            static_assert(decltype(cs)::value == 0 || decltype(cs)::value == 4 || decltype(cs)::value == 8 ||
                              decltype(cs)::value == 16 || decltype(cs)::value == 32,
                          "only the listed sizes and 0 are handed over");
            return (int)decltype(cs)::value;
        });
        const int want = (M == 4 || M == 8 || M == 16 || M == 32) ? M : 0;
        CHECK(got == want, "by_code_size(%d) handed over %d, expected %d", M, got, want);
        CHECK(calls == 1, "by_code_size(%d) called the functor %d times", M, calls);
        CHECK(runtime_code_size_ok(M) == (M % 4 == 0 && M <= 128), "runtime_code_size_ok(%d) = %d", M,
              (int)runtime_code_size_ok(M));
    }
    CHECK(kScanDynLdsMax == 128 * 1024, "kScanDynLdsMax = %zu", kScanDynLdsMax);
    // the result is the functor's, whatever its type
    const double half = by_code_size<4, 8, 16, 32>(16, [](auto cs) { return decltype(cs)::value * 0.5; });
    CHECK(half == 8.0, "by_code_size returned %g for a functor returning 8.0", half);

    const uint32_t word = 0xdeadbeefu;
    const uint32_t *seen = nullptr;
    int calls = 0;
    int arity = with_mask(&word, [&](auto... m) {
        calls++;
        const uint32_t *a[] = {m..., nullptr};
        seen = a[0];
        return (int)sizeof...(m);
    });
    CHECK(arity == 1 && seen == &word && calls == 1, "with_mask(mask): arity %d, calls %d, pointer %s", arity, calls,
          seen == &word ? "kept" : "lost");
    calls = 0;
    arity = with_mask(nullptr, [&](auto... m) {
        calls++;
        return (int)sizeof...(m);
    });
    CHECK(arity == 0 && calls == 1, "with_mask(null): arity %d, calls %d", arity, calls);
    // the pack's type is what a launch site names its kernel with
    with_mask(&word, [](auto... m) {
        static_assert(sizeof...(m) == 0 || (std::is_same<decltype(m), const uint32_t *>::value && ...), "mask type");
        return 0;
    });
    if (failures)
        printf("%d checks failed\n", failures);
    else
        printf("scan_dispatch ok\n");
    return failures ? 1 : 0;
}
