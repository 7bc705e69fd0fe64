// Host check of csrc/plan_math.h (tests/test_plan_math_cpu.py builds it with the address and
// undefined-behaviour sanitizers): the max_codes rules as functions of prefix sums against plain serial loops
// written after the reference's (IndexIVF_HNSW.cpp:267-292, IndexIVF_HNSW_Grouping.cpp:222-262, :283-353), the layout of
// plan_grouping4_kernel's dynamic LDS against the formula and the carving it replaced, and the range of gh_hash.
// Includes nothing else of the library; exit status 0 = every check held.
#include "plan_math.h"

#include <algorithm>
#include <cstdio>
#include <random>
#include <utility>
#include <vector>

using namespace ivfhnsw_gpu_impl;
typedef unsigned long long u64;

static int failures = 0;
#define CHECK(cond, ...)                  \
    do {                                  \
        if (!(cond)) {                    \
            if (failures++ < 20) {        \
                printf("FAIL: " __VA_ARGS__); \
                printf("\n");             \
            }                             \
        }                                 \
    } while (0)

// ---- the reference's loops: the budget is checked after a list is scored
static std::vector<char> serial_ivf_taken(const std::vector<u64> &n, u64 max_codes)
{
    std::vector<char> taken(n.size(), 0);
    u64 ncode = 0;
    for (size_t i = 0; i < n.size(); i++) {
        if (n[i] == 0)
            continue;
        taken[i] = 1;
        ncode += n[i];
        if (ncode >= max_codes)
            break;
    }
    return taken;
}
// rows (non-empty lists) a pass visits when it stops after the row at which the codes seen reach `budget`
static int serial_rows(const std::vector<u64> &n, u64 budget)
{
    int rows = 0;
    u64 ncode = 0;
    for (size_t i = 0; i < n.size(); i++) {
        if (n[i] == 0)
            continue;
        ncode += n[i];
        rows++;
        if (ncode >= budget)
            break;
    }
    return rows;
}

// ---- the same from prefix sums, the way the kernels evaluate them (a lane per list, one scan)
template <class Ends> static int prefix_rows(const std::vector<u64> &n, u64 max_codes, Ends ends)
{
    int upto = 0, first = -1;
    u64 incl = 0;
    for (size_t i = 0; i < n.size(); i++) { // no early exit: every "lane" evaluates its own predicate
        incl += n[i];
        if (n[i] == 0)
            continue;
        upto++;
        if (first < 0 && ends(incl, max_codes))
            first = upto;
    }
    return first >= 0 ? first : upto;
}

static void check_rules(const std::vector<u64> &n, u64 max_codes, const char *what)
{
    const std::vector<char> ref = serial_ivf_taken(n, max_codes);
    u64 incl = 0;
    for (size_t i = 0; i < n.size(); i++) {
        incl += n[i];
        const bool take = plan_takes_list(n[i], incl - n[i], max_codes);
        CHECK(take == (ref[i] != 0), "%s: list %zu of %zu (size %llu, %llu before it), max_codes %llu: taken %d, serial %d", what, i,
              n.size(), n[i], incl - n[i], max_codes, (int)take, (int)ref[i]);
    }
    const int p1 = prefix_rows(n, max_codes, [](u64 in, u64 mc) { return plan_pass1_ends(in, mc); });
    CHECK(p1 == serial_rows(n, 2 * max_codes), "%s: pass 1 rows %d, serial %d (max_codes %llu)", what, p1,
          serial_rows(n, 2 * max_codes), max_codes);
    const int p2 = prefix_rows(n, max_codes, [](u64 in, u64 mc) { return plan_pass2_ends(in, mc); });
    CHECK(p2 == serial_rows(n, max_codes), "%s: pass 2 rows %d, serial %d (max_codes %llu)", what, p2, serial_rows(n, max_codes),
          max_codes);
}

int main()
{
    // ---- 1. the three rules
    std::mt19937_64 rng(20240607);
    const u64 budgets[] = {0, 1, 2, 7, 100, 1000, 65536, 1000000, (u64)1 << 31, (u64)1 << 32, ((u64)1 << 32) + 1, (u64)1 << 36,
                           (u64)1 << 61};
    for (int rep = 0; rep < 400; rep++) {
        const int np = 1 + (int)(rng() % 300);
        // small sizes (budgets bite early), list-sized ones, and sizes whose sums pass 2^32
        const u64 cap = rep % 3 == 0 ? 4 : rep % 3 == 1 ? 3000 : ((u64)1 << 31);
        const int zero_pct = (int)(rng() % 4) * 30; // 0, 30, 60, 90 % empty lists
        std::vector<u64> n(np);
        for (auto &v : n)
            v = (int)(rng() % 100) < zero_pct ? 0 : rng() % (cap + 1);
        u64 sum = 0;
        for (u64 v : n)
            sum += v;
        for (u64 mc : budgets)
            check_rules(n, mc, "random");
        // budgets on and around this query's own sums, where the rules switch
        for (u64 mc : {sum / 4, sum / 2, sum / 2 + 1, sum > 0 ? sum - 1 : 0, sum, sum + 1})
            check_rules(n, mc, "own sums");
    }
    {
        std::vector<u64> big(200, ((u64)1 << 31) - 1); // 200 lists of 2^31 - 1 codes: 4.3e11, beyond 2^32
        u64 sum = 0;
        for (u64 v : big)
            sum += v;
        CHECK(sum > ((u64)1 << 32), "the large case does not pass 2^32");
        for (u64 mc : {(u64)0, (u64)1, (u64)1 << 32, ((u64)1 << 33) + 5, sum / 2, sum, sum + 1})
            check_rules(big, mc, "beyond 2^32");
        check_rules(std::vector<u64>(64, 0), 0, "all empty");
        check_rules(std::vector<u64>(64, 0), 5, "all empty");
        check_rules(std::vector<u64>{0, 0, 9, 0, 1}, 0, "max_codes 0");
        check_rules(std::vector<u64>{0, 0, 9, 0, 1}, 1, "max_codes 1");
    }

    // ---- 2. the layout against the launcher's old formula and the kernel's old carving; 3. no overlap
    for (int d : {16, 32, 96, 128}) {
        for (int nprobe : {1, 64, 200, 1024}) {
            const Plan4Lds l = plan4_lds(d, nprobe);
            const size_t old_shm4 = (size_t)(d + 256) * sizeof(float) + (size_t)nprobe * 8 * sizeof(int);
            CHECK(l.bytes() == old_shm4, "d %d nprobe %d: %zu bytes, before %zu", d, nprobe, l.bytes(), old_shm4);
            // s_dist = s_q + d + wave * 64; s_rowp = s_q + d + 256; then seven more arrays of nprobe words, in this order
            const Plan4Row order[] = {kRowProbe, kRowCentroid, kRowSize, kRowAlpha, kRowNorm, kRowFirstCode, kRowCoarseDist, kRowActive};
            CHECK(sizeof(order) / sizeof(order[0]) == kPlan4Rows, "a Plan4Row is missing from the check");
            CHECK(l.dist == (uint32_t)d, "d %d: dist at word %u", d, l.dist);
            // [offset, offset + length) of every array, sorted by offset: disjoint and inside the total
            std::vector<std::pair<uint32_t, uint32_t>> a = {{0u, (uint32_t)d}, {l.dist, 4 * 64}};
            for (int i = 0; i < 8; i++) {
                const uint32_t before = (uint32_t)d + 256 + (uint32_t)i * (uint32_t)nprobe;
                CHECK(l.row(order[i]) == before, "d %d nprobe %d: row array %d at word %u, before %u", d, nprobe, i, l.row(order[i]), before);
                a.push_back({l.row(order[i]), (uint32_t)nprobe});
            }
            std::sort(a.begin(), a.end());
            for (size_t i = 0; i + 1 < a.size(); i++)
                CHECK(a[i].first + a[i].second <= a[i + 1].first, "d %d nprobe %d: arrays at words %u (+%u) and %u overlap", d, nprobe,
                      a[i].first, a[i].second, a[i + 1].first);
            CHECK(a.back().first + a.back().second <= l.words, "d %d nprobe %d: the last array ends beyond the total", d, nprobe);
            CHECK(l.dist % 4 == 0, "d %d: the query's float4 reads need dist at a multiple of 16 bytes", d);
        }
    }

    // ---- gh_hash addresses the slots, all of them
    CHECK((GH_SLOTS & (GH_SLOTS - 1)) == 0 && GH_PROBES > 0 && GH_PROBES <= GH_SLOTS, "hash set constants");
    std::vector<char> seen(GH_SLOTS, 0);
    for (uint32_t id = 0; id < (1u << 20); id++) {
        const uint32_t h = gh_hash(id);
        CHECK(h < (uint32_t)GH_SLOTS, "gh_hash(%u) = %u", id, h);
        if (h < (uint32_t)GH_SLOTS)
            seen[h] = 1;
    }
    for (uint32_t id : {0x7fffffffu, 0x80000000u, 0xfffffffeu, GH_EMPTY})
        CHECK(gh_hash(id) < (uint32_t)GH_SLOTS, "gh_hash(%u) = %u", id, gh_hash(id));
    CHECK(std::count(seen.begin(), seen.end(), 1) == GH_SLOTS, "gh_hash leaves slots unused");

    if (failures)
        printf("%d checks failed\n", failures);
    else
        printf("plan_math ok\n");
    return failures ? 1 : 0;
}
