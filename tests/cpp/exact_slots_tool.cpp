// The host arithmetic of the base filter slots (csrc/sweep_plan_math.h) on the host, under the address and
// undefined-behaviour sanitizers: the strip bound, the strip layout from the 34 counts and the per-strip split cut.  Built
// and run by tests/test_exact_slots_plan_cpu.py.
#include "sweep_plan_math.h"

#include <cstdio>
#include <cstdlib>
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

// the queries of a chunk with these counts per bucket laid out as the device lays them out (count, layout, scatter), then:
// every strip of one bucket, every query with a strip in exactly one row, the others in none, the forms in contiguous ranges
static void check_layout(const std::vector<uint32_t> &counts, const std::vector<uint32_t> &forms)
{
    size_t m = 0;
    for (uint32_t c : counts)
        m += c;
    // the bytes of the queries, bucket by bucket, then shuffled
    std::vector<uint8_t> bytes;
    for (int b = 0; b < kStripBuckets; b++)
        for (uint32_t i = 0; i < counts[b]; i++)
            bytes.push_back(b < kStripSlots ? (uint8_t)b : b == kStripNone ? (uint8_t)0xff : (uint8_t)(32 + (i * 7) % 223));
    std::mt19937 rng((unsigned)m * 2654435761u + counts[0]);
    for (size_t i = bytes.size(); i > 1; i--)
        std::swap(bytes[i - 1], bytes[rng() % i]);

    // count, as strip_count_kernel: a byte whose entry sweeps nothing goes to the invalid bucket
    auto bucket = [&](uint8_t byte) {
        const int b = sweep_strip_bucket(byte);
        return b != kStripInvalid && forms[b] == kSweepColsNothing ? kStripInvalid : b;
    };
    uint32_t cnt[kStripBuckets] = {};
    for (uint8_t byte : bytes)
        cnt[bucket(byte)]++;
    StripLayout lay;
    sweep_strip_layout(cnt, forms.data(), &lay);

    const size_t bound = sweep_strip_bound(m);
    CHECK(lay.nstrips <= bound);
    CHECK(bound == m / 32 + 33);
    std::vector<int> strip_slot(bound, -1);
    std::vector<int32_t> rows(bound * 32, -1);
    uint32_t cursor[kStripBuckets] = {};
    for (int b = 0; b <= kStripNone; b++) {
        if (lay.first[b] == ~0u) {
            CHECK(cnt[b] == 0 || forms[b] == kSweepColsNothing);
            continue;
        }
        for (uint32_t i = 0; i < (cnt[b] + 31) / 32; i++) {
            CHECK(lay.first[b] + i < lay.nstrips);
            CHECK(strip_slot[lay.first[b] + i] == -1); // no strip belongs to two buckets
            strip_slot[lay.first[b] + i] = b;
        }
    }
    CHECK(lay.first[kStripInvalid] == ~0u);
    for (size_t q = 0; q < bytes.size(); q++) {
        const int b = bucket(bytes[q]);
        if (lay.first[b] == ~0u)
            continue;
        const uint32_t pos = cursor[b]++;
        CHECK(pos < cnt[b]);
        CHECK((size_t)lay.first[b] * 32 + pos < rows.size());
        rows[(size_t)lay.first[b] * 32 + pos] = (int32_t)q;
    }
    // every strip below nstrips has a bucket, is slot-uniform, lies in its form's range; the ranges are contiguous and in order
    CHECK(lay.range[0][0] == 0 && lay.range[0][1] == lay.range[1][0] && lay.range[1][1] == lay.range[2][0] &&
          lay.range[2][1] == lay.nstrips);
    std::vector<int> seen(bytes.size(), 0);
    for (uint32_t s = 0; s < lay.nstrips; s++) {
        const int b = strip_slot[s];
        CHECK(b >= 0);
        if (b < 0)
            continue;
        const uint32_t f = forms[b];
        CHECK(f < 3 && lay.range[f][0] <= s && s < lay.range[f][1]);
        int real = 0;
        for (int i = 0; i < 32; i++) {
            const int32_t q = rows[(size_t)s * 32 + i];
            if (q < 0)
                continue;
            real++;
            CHECK(bucket(bytes[q]) == b);
            seen[q]++;
        }
        CHECK(real > 0); // no strip of padding alone
    }
    for (size_t s = lay.nstrips; s < bound; s++)
        for (int i = 0; i < 32; i++)
            CHECK(rows[s * 32 + i] == -1);
    for (size_t q = 0; q < bytes.size(); q++) {
        const int b = bucket(bytes[q]);
        CHECK(seen[q] == (b == kStripInvalid ? 0 : 1));
    }
}

static std::vector<uint32_t> some_forms(std::mt19937 &rng)
{
    std::vector<uint32_t> f(kStripNone + 1);
    for (int b = 0; b < kStripSlots; b++)
        f[b] = 1 + rng() % 3; // Masked, Indirect or nothing
    f[kStripNone] = kSweepColsDense;
    return f;
}

int main()
{
    std::mt19937 rng(20260101);
    // seeded count vectors over the 34 buckets, m <= 200
    for (int t = 0; t < 3000; t++) {
        std::vector<uint32_t> counts(kStripBuckets, 0);
        const int m = (int)(rng() % 201);
        const int spread = 1 + (int)(rng() % kStripBuckets);
        for (int i = 0; i < m; i++)
            counts[rng() % spread + (rng() % 4 == 0 ? kStripBuckets - spread : 0)]++;
        check_layout(counts, some_forms(rng));
    }
    // the hand-written ones
    std::vector<uint32_t> all_set(kStripNone + 1, kSweepColsMasked);
    all_set[kStripNone] = kSweepColsDense;
    for (int b = 0; b < kStripSlots; b += 2)
        all_set[b] = kSweepColsIndirect;
    for (int b = 0; b < kStripBuckets; b++) { // all in one bucket
        std::vector<uint32_t> c(kStripBuckets, 0);
        c[b] = 200;
        check_layout(c, all_set);
    }
    check_layout(std::vector<uint32_t>(kStripBuckets, 1), all_set); // one query per bucket
    {
        std::vector<uint32_t> c(kStripBuckets, 0);
        c[0] = 31, c[1] = 32, c[2] = 33, c[kStripNone] = 33, c[kStripInvalid] = 31;
        check_layout(c, all_set);
    }
    {
        std::vector<uint32_t> c(kStripBuckets, 0); // all invalid: by byte, and by slots that sweep nothing
        c[kStripInvalid] = 200;
        check_layout(c, all_set);
        std::vector<uint32_t> nothing(kStripNone + 1, kSweepColsNothing);
        nothing[kStripNone] = kSweepColsDense;
        std::vector<uint32_t> c2(kStripBuckets, 5);
        c2[kStripNone] = 0;
        check_layout(c2, nothing);
    }
    // the bound is reached: 33 buckets of 1 query beyond whole strips
    {
        std::vector<uint32_t> c(kStripBuckets, 0);
        for (int b = 0; b <= kStripNone; b++)
            c[b] = 1;
        uint32_t forms[kStripNone + 1], cnt[kStripBuckets] = {};
        for (int b = 0; b <= kStripNone; b++)
            forms[b] = all_set[b], cnt[b] = c[b];
        StripLayout lay;
        sweep_strip_layout(cnt, forms, &lay);
        CHECK(lay.nstrips == 33 && sweep_strip_bound(33) == 34);
    }

    // the per-strip split cut: the cuts of every nsplit tile [0, nx) in order, in whole tiles of 32
    for (size_t nx : {(size_t)0, (size_t)1, (size_t)31, (size_t)32, (size_t)33, (size_t)6001})
        for (int nsplit = 1; nsplit <= 64; nsplit++) {
            size_t at = 0;
            for (int s = 0; s < nsplit; s++) {
                size_t b, e;
                sweep_split_cut(nx, nsplit, s, &b, &e);
                CHECK(b == at && e >= b && e <= nx);
                CHECK(b % 32 == 0 || b == nx);
                CHECK(e % 32 == 0 || e == nx);
                // what the kernels compute from cols_per_split
                const size_t cps = sweep_cols_per_split(nx, nsplit);
                const size_t kb = (size_t)s * cps < nx ? (size_t)s * cps : nx, ke = kb + cps < nx ? kb + cps : nx;
                CHECK(kb == b && ke == e);
                at = e;
            }
            CHECK(at == nx);
        }
    if (fails)
        return 1;
    printf("exact_slots ok\n");
    return 0;
}
