// The host arithmetic of the base values (csrc/sweep_plan_math.h) on the host, under the address and
// undefined-behaviour sanitizers: the window of an interval against a linear scan over the cross product of DESIGN.md
// 3.24's eleven boundary values (and random intervals) on stores of values in (value, row) order, the strip bound against
// the plan restated step by step, and the chunk rule of the k-search.  Built and run by tests/test_exact_values_cpu.py.
#include "sweep_plan_math.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <random>
#include <vector>

using namespace ivfhnsw_gpu_impl;

static int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);         \
            fails++;                                                    \
        }                                                               \
    } while (0)

static const uint32_t kEdge[] = {0u, 1u, 76u, 77u, 78u, 0xffffu, 0x10000u, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};

// vals: a value per row.  The window of (lo, hi) in the order by (value, row) against the rows lo <= v <= hi counted one by one.
static void check_window(const std::vector<uint32_t> &vals, const std::vector<uint32_t> &order, uint32_t lo, uint32_t hi)
{
    const uint32_t n = (uint32_t)vals.size();
    uint32_t a = 123, b = 456;
    sweep_value_window([&](uint32_t i) { return vals[order[i]]; }, n, lo, hi, &a, &b);
    CHECK(a <= b && b <= n);
    uint32_t pass = 0;
    for (uint32_t r = 0; r < n; r++)
        pass += lo <= vals[r] && vals[r] <= hi ? 1u : 0u;
    CHECK(b - a == pass);
    for (uint32_t i = 0; i < n; i++) {
        const uint32_t v = vals[order[i]];
        CHECK((lo <= v && v <= hi) == (a <= i && i < b));
    }
    if (lo > hi)
        CHECK(a == 0 && b == 0);
    // a store without a value array: every row reads 0xffffffff
    sweep_value_window([](uint32_t) { return 0xffffffffu; }, n, lo, hi, &a, &b);
    CHECK(a == 0 && b == (lo <= hi && hi == 0xffffffffu ? n : 0u));
}

// The plan of a chunk as the device builds it from the windows: keys, the stable order, Dense strips first, windowed
// strips of 32 in the order of their starts, each spanning [A, B) with its rows' windows relative to A.  Returns the strips.
static size_t check_plan(const std::vector<uint32_t> &wa, const std::vector<uint32_t> &wb, uint32_t n)
{
    const size_t m = wa.size(), bound = sweep_value_strip_bound(m);
    std::vector<uint32_t> keys(m), sorted(m);
    uint32_t nfull = 0, nwin = 0;
    for (size_t q = 0; q < m; q++) {
        const bool none = wa[q] >= wb[q], full = !none && wa[q] == 0 && wb[q] == n;
        keys[q] = none ? 0xffffffffu : full ? 0u : wa[q] + 1u;
        nfull += full;
        nwin += !none && !full;
    }
    std::iota(sorted.begin(), sorted.end(), 0u);
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    const size_t dense = (nfull + 31) / 32, all = dense + (nwin + 31) / 32;
    CHECK(all <= bound);
    std::vector<int> seen(m, 0);
    for (size_t i = 0; i < (size_t)nfull + nwin; i++) {
        const uint32_t q = sorted[i];
        seen[q]++;
        if (i < nfull) {
            CHECK(wa[q] == 0 && wb[q] == n);
            continue;
        }
        const size_t j = i - nfull, j0 = nfull + (j & ~(size_t)31), j1 = std::min<size_t>(j0 + 32, (size_t)nfull + nwin);
        const uint32_t A = wa[sorted[j0]];
        uint32_t B = 0;
        for (size_t t = j0; t < j1; t++) {
            CHECK(wa[sorted[t]] >= A); // the strip's first query has its smallest start
            B = std::max(B, wb[sorted[t]]);
        }
        CHECK(wa[q] < wb[q] && wa[q] - A < wb[q] - A && wb[q] - A <= B - A && B <= n);
        CHECK(dense + j / 32 < all);
    }
    for (size_t i = (size_t)nfull + nwin; i < m; i++)
        CHECK(wa[sorted[i]] >= wb[sorted[i]]); // the queries that get no strip: their windows are empty
    for (size_t q = 0; q < m; q++)
        CHECK(seen[q] == (wa[q] < wb[q] ? 1 : 0));
    return all;
}

int main()
{
    std::mt19937 rng(12345);
    // ---- the window function
    for (int round = 0; round < 6; round++) {
        const uint32_t n = round == 0 ? 1 : round == 1 ? 33 : 200 + 57 * round;
        std::vector<uint32_t> vals(n);
        for (uint32_t r = 0; r < n; r++) {
            const uint32_t pick = rng() % 4;
            vals[r] = round == 2   ? 0xffffffffu                                  // no row holds a value
                      : round == 3 ? 77u                                          // one long run
                      : pick == 0  ? kEdge[rng() % 11]
                      : pick == 1  ? 0x7fffff00u + rng() % 512
                      : pick == 2  ? 1000u + rng() % 4
                                   : (uint32_t)rng();
        }
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return vals[x] < vals[y]; });
        for (uint32_t lo : kEdge)
            for (uint32_t hi : kEdge)
                check_window(vals, order, lo, hi);
        for (int i = 0; i < 200; i++) {
            const uint32_t x = i % 2 ? vals[rng() % n] : (uint32_t)rng(), y = i % 3 ? vals[rng() % n] : (uint32_t)rng();
            check_window(vals, order, x, y);
            check_window(vals, order, y, x);
        }
    }
    { // the empty store
        uint32_t a = 1, b = 1;
        sweep_value_window([](uint32_t) { return 0u; }, 0, 0, 0xffffffffu, &a, &b);
        CHECK(a == 0 && b == 0);
    }

    // ---- the strip bound, against the plan restated
    CHECK(sweep_value_strip_bound(1) == 2 && sweep_value_strip_bound(32) == 3 && sweep_value_strip_bound(33) == 3 &&
          sweep_value_strip_bound(kExactChunk) == kExactChunk / 32 + 2);
    for (int round = 0; round < 300; round++) {
        const size_t m = round < 70 ? (size_t)round + 1 : 1 + rng() % 700;
        const uint32_t n = 1 + rng() % 5000;
        std::vector<uint32_t> wa(m), wb(m);
        const int mode = round % 5;
        for (size_t q = 0; q < m; q++) {
            const uint32_t pick = mode == 0 ? 0 : mode == 1 ? 1 : mode == 2 ? 2 : rng() % 3;
            if (pick == 0) { // the whole store
                wa[q] = 0;
                wb[q] = n;
            } else if (pick == 1) { // empty
                wa[q] = wb[q] = rng() % (n + 1);
            } else {
                wa[q] = rng() % n;
                wb[q] = wa[q] + 1 + rng() % (n - wa[q]);
            }
        }
        const size_t strips = check_plan(wa, wb, n);
        CHECK(strips <= sweep_value_strip_bound(m));
    }
    { // the bound is met: 1 whole-store query and 32 k + 1 windowed ones
        std::vector<uint32_t> wa(34, 5), wb(34, 9);
        wa[0] = 0;
        wb[0] = 100;
        CHECK(check_plan(wa, wb, 100) == 3 && sweep_value_strip_bound(34) == 3);
    }

    // ---- the chunk rule of the k-search: within the partial tables' bytes, a multiple of 128 never below 128, the largest
    for (int nsplit : {1, 2, 3, 7, 16, 33, 64})
        for (size_t k : {(size_t)1, (size_t)10, (size_t)32, (size_t)33, (size_t)100}) {
            const size_t c = sweep_value_chunk(nsplit, k);
            const size_t per_strip = (size_t)nsplit * 32 * k * sizeof(uint64_t);
            CHECK(c >= 128 && c <= kExactChunk && c % 128 == 0);
            CHECK(per_strip * sweep_value_strip_bound(c) <= kExactPartBytes);
            if (c < kExactChunk)
                CHECK(per_strip * sweep_value_strip_bound(c + 128) > kExactPartBytes);
        }
    CHECK(sweep_value_chunk(1, 1) == kExactChunk);
    CHECK(sweep_value_chunk(64, 100) < kExactChunk);
    CHECK(sweep_value_plan_bytes(3) == sweep_tag_plan_bytes(3) + 3 * 32 * sizeof(StripWin) && sizeof(StripWin) == 8);

    if (fails) {
        printf("%d checks failed\n", fails);
        return 1;
    }
    printf("exact_values ok\n");
    return 0;
}
