// The host arithmetic of the base tags (csrc/sweep_plan_math.h) on the host, under the address and
// undefined-behaviour sanitizers: the strip bound against brute-force counts, the chunk rule of the k-search, the plan's
// layout restated step by step (keys, stable order, the two scans, scatter) and the per-strip split cut.  Built and run
// by tests/test_exact_tags_plan_cpu.py.
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

// The plan of a chunk as the device builds it: bucket 0 = "none", bucket t + 1 = tag t; the queries in the stable order by
// bucket; a bucket's strips where it sweeps something.  rows_of[t] = the rows tag t holds, n = the rows of the store.
// Returns the strips taken.
static size_t check_plan(const std::vector<uint16_t> &qtags, const std::vector<uint32_t> &rows_of, uint32_t n, size_t tags_in_use)
{
    const size_t m = qtags.size(), bound = sweep_tag_strip_bound(m, tags_in_use);
    std::vector<uint32_t> keys(m), qcnt(kTagValues + 1, 0), nstr(kTagValues + 1, 0);
    for (size_t q = 0; q < m; q++) {
        keys[q] = ((uint32_t)qtags[q] + 1u) & 0xffffu;
        qcnt[keys[q]]++;
    }
    for (size_t b = 0; b < kTagValues; b++)
        if (qcnt[b] && (b == 0 ? n != 0 : rows_of[b - 1] != 0))
            nstr[b] = (qcnt[b] + 31) / 32;
    std::vector<uint32_t> sorted(m);
    std::iota(sorted.begin(), sorted.end(), 0u);
    std::stable_sort(sorted.begin(), sorted.end(), [&](uint32_t a, uint32_t b) { return keys[a] < keys[b]; });
    std::vector<uint32_t> qoff(kTagValues + 1), sfirst(kTagValues + 1);
    std::exclusive_scan(qcnt.begin(), qcnt.end(), qoff.begin(), 0u);
    std::exclusive_scan(nstr.begin(), nstr.end(), sfirst.begin(), 0u);
    const size_t nstrips = sfirst[kTagValues], dense = sfirst[1];
    CHECK(nstrips <= bound);
    std::vector<int32_t> srow(bound * 32, -1);
    std::vector<int> stag(bound, -2);
    for (size_t i = 0; i < m; i++) {
        const uint32_t q = sorted[i], b = keys[q], pos = (uint32_t)i - qoff[b];
        if (sfirst[b + 1] == sfirst[b])
            continue;
        const size_t strip = sfirst[b] + pos / 32;
        CHECK(strip < nstrips);
        if (strip >= bound)
            continue;
        CHECK(srow[strip * 32 + pos % 32] == -1);
        srow[strip * 32 + pos % 32] = (int32_t)q;
        if (pos % 32 == 0) {
            CHECK(stag[strip] == -2);
            stag[strip] = (int)b - 1; // -1: none
        }
    }
    std::vector<int> seen(m, 0);
    for (size_t s = 0; s < nstrips && s < bound; s++) {
        CHECK(stag[s] != -2);                  // every strip has an entry
        CHECK((stag[s] == -1) == (s < dense)); // the Dense strips first
        CHECK(srow[s * 32] >= 0);
        int32_t last = -1;
        for (int i = 0; i < 32; i++) {
            const int32_t q = srow[s * 32 + i];
            if (q < 0)
                continue;
            CHECK(q > last || i == 0); // the stable order: ascending query inside a strip
            last = q;
            CHECK((qtags[q] == kTagNone ? -1 : (int)qtags[q]) == stag[s]);
            seen[q]++;
        }
    }
    for (size_t s = nstrips; s < bound; s++)
        for (int i = 0; i < 32; i++)
            CHECK(srow[s * 32 + i] == -1);
    for (size_t q = 0; q < m; q++)
        CHECK(seen[q] == ((qtags[q] == kTagNone ? n != 0 : rows_of[qtags[q]] != 0) ? 1 : 0));
    // ... and the brute-force count
    size_t brute = 0;
    for (size_t b = 0; b < kTagValues; b++)
        brute += nstr[b];
    CHECK(brute == nstrips);
    return nstrips;
}

int main()
{
    std::mt19937 rng(20260322);
    // random histograms: T tags in use out of 65535, m <= 16384 queries over "none", tags with rows and tags without
    for (int t = 0; t < 400; t++) {
        const size_t T = t % 7 == 0 ? rng() % 65536 : t % 7 == 1 ? 0 : rng() % 2000;
        const size_t m = t % 5 == 0 ? 1 + rng() % 16384 : 1 + rng() % 700;
        std::vector<uint32_t> rows_of(kTagValues, 0);
        std::vector<uint16_t> used;
        while (used.size() < T) { // T distinct tags below 0xffff
            const uint16_t x = (uint16_t)(rng() % 65535);
            if (!rows_of[x]) {
                rows_of[x] = 1 + rng() % 9;
                used.push_back(x);
            }
        }
        const size_t spread = 1 + rng() % (used.size() + 1);
        std::vector<uint16_t> qtags(m);
        for (size_t q = 0; q < m; q++) {
            const unsigned r = rng() % 16;
            qtags[q] = r == 0 || used.empty() ? (uint16_t)kTagNone : r == 1 ? (uint16_t)(rng() % 65535) : used[rng() % spread % used.size()];
        }
        CHECK(check_plan(qtags, rows_of, 1000, T) <= m / 32 + std::min(m, T + 1));
    }
    // the bound is reached: T + 1 buckets of one query beyond whole strips
    {
        std::vector<uint32_t> rows_of(kTagValues, 0);
        std::vector<uint16_t> qtags;
        for (int t = 0; t < 40; t++) {
            rows_of[t * 1000] = 4;
            qtags.push_back((uint16_t)(t * 1000));
        }
        qtags.push_back((uint16_t)kTagNone);
        for (int i = 0; i < 64; i++)
            qtags.push_back(0); // two whole strips more of tag 0: 33 queries in all -> 3 strips
        CHECK(check_plan(qtags, rows_of, 77, 40) == 40 + 1 + 2);
        CHECK(sweep_tag_strip_bound(qtags.size(), 40) == 105 / 32 + 41);
        CHECK(sweep_tag_strip_bound(5, 65535) == 0 + 5 && sweep_tag_strip_bound(16384, 0) == 512 + 1);
        // an empty store: "none" sweeps nothing either; no tag array: only "none" has strips
        CHECK(check_plan(qtags, std::vector<uint32_t>(kTagValues, 0), 0, 0) == 0);
        CHECK(check_plan(qtags, std::vector<uint32_t>(kTagValues, 0), 77, 0) == 1);
    }

    // the chunk rule: a multiple of 128 in [128, kExactChunk], the partial tables over the padded rows within kExactPartBytes,
    // and the largest such
    auto part_bytes = [](int nsplit, size_t k, size_t chunk, size_t T) {
        return (size_t)nsplit * sweep_tag_strip_bound(chunk, T) * 32 * k * sizeof(uint64_t);
    };
    for (int nsplit : {1, 2, 3, 7, 16, 33, 64})
        for (size_t k : {(size_t)1, (size_t)10, (size_t)16, (size_t)32, (size_t)33, (size_t)100})
            for (size_t T : {(size_t)0, (size_t)1, (size_t)32, (size_t)154, (size_t)155, (size_t)305, (size_t)1024, (size_t)20000, (size_t)65535}) {
                const size_t c = sweep_tag_chunk(nsplit, k, T);
                CHECK(c >= 128 && c <= kExactChunk && c % 128 == 0);
                CHECK(part_bytes(nsplit, k, c, T) <= kExactPartBytes);
                CHECK(c == kExactChunk || part_bytes(nsplit, k, c + 128, T) > kExactPartBytes);
            }
    // what the test of more than one chunk relies on: k = 100 under 64 splits falls to 128 queries from 155 tags on
    CHECK(sweep_tag_chunk(64, 100, 154) == 256 && sweep_tag_chunk(64, 100, 155) == 128 && sweep_tag_chunk(64, 100, 305) == 128);
    CHECK(sweep_tag_chunk(1, 1, 65535) == kExactChunk);

    // the per-strip split cut over a tag's short list: the cuts tile [0, nx) in order, in whole tiles of 32
    for (size_t nx = 1; nx <= 100; nx++)
        for (int nsplit : {1, 3, 64}) {
            size_t at = 0;
            int nonempty = 0;
            for (int s = 0; s < nsplit; s++) {
                size_t b, e;
                sweep_split_cut(nx, nsplit, s, &b, &e);
                CHECK(b == at && e >= b && e <= nx);
                CHECK(b % 32 == 0 || b == nx);
                CHECK(e % 32 == 0 || e == nx);
                nonempty += e > b;
                at = e;
            }
            CHECK(at == nx);
            CHECK(nonempty <= (int)((nx + 31) / 32)); // at 64 splits of a 4-row tag all but one are empty
        }
    if (fails)
        return 1;
    printf("exact_tags ok\n");
    return 0;
}
