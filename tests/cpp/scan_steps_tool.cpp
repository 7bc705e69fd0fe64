// Host check of csrc/scan_plan_math.h (tests/test_scan_steps_cpu.py builds it with the address and undefined-behaviour
// sanitizers): the index arithmetic the ADC scan kernels share, on seeded random plans, against a linear reference --
// the slices of a query, the three segment seeks over a staged chunk, and the chunks of the bitmap form.  Includes
// nothing else of the library; exit status 0 = every check held.
#include "scan_plan_math.h"

#include <algorithm>
#include <cstdio>
#include <vector>

using namespace ivfhnsw_gpu_impl;

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

static uint64_t rng_state;
static uint32_t rnd(uint32_t n) // [0, n)
{
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((rng_state >> 33) % n);
}

struct Plan {
    std::vector<uint32_t> lpos; // [nseg]
    std::vector<uint32_t> seg;  // [total]: the linear reference, the segment of every position
    uint32_t nseg, total;
};

// lengths mixing 1, ~16 and ~1000, and one segment longer than the bitmap span
static Plan make_plan(uint32_t nseg, uint64_t seed)
{
    rng_state = seed;
    Plan p;
    p.nseg = nseg;
    const uint32_t big = rnd(nseg);
    uint32_t pos = 0;
    for (uint32_t i = 0; i < nseg; i++) {
        const uint32_t kind = rnd(256);
        uint32_t len = kind < 128 ? 1u : kind < 255 ? 8u + rnd(17) : 900u + rnd(200);
        if (i == big)
            len = (uint32_t)kBmSpanCap + 1u + rnd(100);
        p.lpos.push_back(pos);
        p.seg.insert(p.seg.end(), len, i);
        pos += len;
    }
    p.total = pos;
    return p;
}

// Every position of the plan, staged in chunks of `cap` segments as a kernel stages them, walked upward from earlier
// segments of its chunk: the policy's answer is the reference's.  `full`: from EVERY earlier segment.  Otherwise that
// product is taken for the first and the last position of every segment only -- a policy reads p in comparisons with
// entries of s_lpos and nowhere else, so from the same s every position of a segment takes the path of those two --
// and the positions between them start from the chunk's first segment, from their own, and from the one a lane that
// strides by 256 positions was in before.  (The whole product at cap 1024 is 10^9 steps of the linear policy.)
template <class Policy> static void check_seek(const Plan &pl, uint32_t cap, bool full, const char *name)
{
    std::vector<uint32_t> s_lpos(cap + 1);
    for (uint32_t cs = 0; cs < pl.nseg; cs += cap) {
        const uint32_t cn = scan_umin(cap, pl.nseg - cs);
        const uint32_t ch = plan_chunk_end(pl.lpos.data(), cs, cn, pl.nseg, pl.total);
        std::copy(pl.lpos.begin() + cs, pl.lpos.begin() + cs + cn, s_lpos.begin());
        s_lpos[cn] = ch;
        CHECK(ch == (cs + cn == pl.nseg ? pl.total : pl.lpos[cs + cn]), "plan_chunk_end(%u, %u) = %u", cs, cn, ch);
        const uint32_t cl = s_lpos[0];
        for (uint32_t p = cl; p < ch; p++) {
            const uint32_t want = pl.seg[p] - cs;
            const bool edge = p == s_lpos[want] || p + 1 == s_lpos[want + 1];
            const uint32_t few[3] = {0, want, p - cl >= 256 ? pl.seg[p - 256] - cs : 0};
            const bool all = full || edge;
            for (uint32_t i = 0; i < (all ? want + 1 : 3u); i++) {
                const uint32_t s = all ? i : few[i];
                const uint32_t got = Policy::seek(s_lpos.data(), s, cn, p);
                if (got != want) {
                    CHECK(false, "%s cap %u nseg %u: position %u from s = %u gave %u, expected %u", name, cap, pl.nseg, p, s,
                          got, want);
                    return;
                }
            }
        }
    }
}

static void check_slices_and_bitmap(const Plan &pl, int nsplit, int threads)
{
    std::vector<uint8_t> seen(pl.total, 0);
    uint32_t prev_hi = 0;
    for (int split = 0; split < nsplit; split++) {
        const ScanSlice sl = scan_slice(pl.total, nsplit, split, threads);
        CHECK(sl.lo <= sl.hi && sl.hi <= pl.total, "slice %d/%d: [%u, %u) of %u", split, nsplit, sl.lo, sl.hi, pl.total);
        CHECK(sl.lo == prev_hi, "slice %d/%d starts at %u, the one before ended at %u", split, nsplit, sl.lo, prev_hi);
        CHECK(sl.lo % threads == 0 || sl.lo == pl.total, "slice %d/%d starts at %u, no multiple of %d", split, nsplit, sl.lo,
              threads);
        CHECK((sl.hi - sl.lo) % threads == 0 || sl.hi == pl.total, "slice %d/%d: %u positions and not the last", split, nsplit,
              sl.hi - sl.lo);
        prev_hi = sl.hi;
        if (sl.lo >= sl.hi)
            continue; // the kernels return here
        const uint32_t lo = sl.lo, hi = sl.hi;

        // the bitmap form's walk over this slice, chunk by chunk
        uint32_t cs = first_segment(pl.lpos.data(), pl.nseg, lo);
        CHECK(cs == pl.seg[lo], "first_segment(lo = %u) = %u, expected %u", lo, cs, pl.seg[lo]);
        while (cs < pl.nseg) {
            const uint32_t cl = pl.lpos[cs];
            if (cl >= hi)
                break;
            const BitmapExtent e = bitmap_extent(pl.lpos.data(), cs, pl.nseg, pl.total);
            CHECK(e.cn >= 1 && e.cn <= (uint32_t)kBmSegCap && cs + e.cn <= pl.nseg, "chunk at %u: %u segments", cs, e.cn);
            if (e.cn < 1 || cs + e.cn > pl.nseg)
                return;
            CHECK(e.ch == (cs + e.cn == pl.nseg ? pl.total : pl.lpos[cs + e.cn]), "chunk at %u: end %u", cs, e.ch);
            CHECK(e.single == (e.ch - cl > (uint32_t)kBmSpanCap), "chunk at %u: single %d over %u positions", cs, (int)e.single,
                  e.ch - cl);
            CHECK(!e.single || e.cn == 1, "chunk at %u: %u segments span %u positions", cs, e.cn, e.ch - cl);
            CHECK(e.nwords == (e.single ? 0u : (e.ch - cl + 63) / 64) && e.nwords <= (uint32_t)kBmSpanWords,
                  "chunk at %u: %u words", cs, e.nwords);
            // greedy: one more segment would not have fitted
            if (!e.single && e.cn < (uint32_t)kBmSegCap && cs + e.cn < pl.nseg) {
                const uint32_t next_end = cs + e.cn + 1 == pl.nseg ? pl.total : pl.lpos[cs + e.cn + 1];
                CHECK(next_end - cl > (uint32_t)kBmSpanCap, "chunk at %u stops at %u segments with room left", cs, e.cn);
            }
            // mask and prefix as the kernels build them
            unsigned long long mask[kBmSpanWords] = {};
            uint32_t pref[kBmSpanWords] = {};
            if (!e.single) {
                for (uint32_t i = 0; i < e.cn; i++) {
                    const uint32_t r = pl.lpos[cs + i] - cl;
                    mask[r >> 6] |= 1ull << (r & 63);
                }
                uint32_t run = 0;
                for (uint32_t w = 0; w < e.nwords; w++) {
                    pref[w] = run;
                    run += (uint32_t)__builtin_popcountll(mask[w]);
                }
            }
            const uint32_t b0 = std::max(cl, lo), b1 = std::min(e.ch, hi);
            for (uint32_t p = b0; p < b1; p++) {
                const uint32_t r = p - cl, wi = r >> 6;
                const int lane = (int)(r & 63);
                uint32_t sgi = 0;
                if (!e.single) {
                    const uint32_t below = (uint32_t)__builtin_popcountll(mask[wi] & ((1ull << lane) - 1ull));
                    sgi = bitmap_segment(pref[wi], mask[wi], below, lane);
                }
                CHECK(cs + sgi == pl.seg[p], "segment_of(position %u) = %u, expected %u (chunk at %u)", p, cs + sgi,
                      pl.seg[p], cs);
                seen[p]++;
            }
            cs += e.cn;
        }
    }
    CHECK(prev_hi == pl.total, "the %d slices end at %u of %u", nsplit, prev_hi, pl.total);
    uint32_t bad = 0;
    for (uint32_t p = 0; p < pl.total; p++)
        bad += seen[p] != 1;
    CHECK(bad == 0, "nseg %u nsplit %d: %u positions not covered exactly once by the bitmap chunks", pl.nseg, nsplit, bad);
}

int main()
{
    static_assert(kBmSegCap == 256 && kBmSpanCap == 8192 && kBmSpanWords == 128, "the bitmap form's one set of constants");
    const uint32_t nsegs[] = {1, 2, 63, 64, 65, 255, 256, 257, 1024};
    uint64_t seed = 0x5ca9;
    for (uint32_t nseg : nsegs) {
        const Plan pl = make_plan(nseg, seed++);
        // all three on the same chunks of 64 (k1, tail), then each at the larger caps its kernels stage
        check_seek<SeekLinear>(pl, 64, true, "SeekLinear");
        check_seek<SeekStep2Halves>(pl, 64, true, "SeekStep2Halves");
        check_seek<SeekHalves>(pl, 64, true, "SeekHalves");
        check_seek<SeekStep2Halves>(pl, 256, false, "SeekStep2Halves"); // k1, range
        check_seek<SeekStep2Halves>(pl, 1024, false, "SeekStep2Halves"); // k1
        check_seek<SeekHalves>(pl, 256, false, "SeekHalves"); // heap
        check_seek<SeekHalves>(pl, 512, false, "SeekHalves"); // topk
        for (int nsplit : {1, 3, 32})
            check_slices_and_bitmap(pl, nsplit, 256);
    }
    // a chunk that fills the span to the position: 128 segments of 64
    {
        Plan pl;
        pl.nseg = 300;
        for (uint32_t i = 0; i < pl.nseg; i++) {
            pl.lpos.push_back(64 * i);
            pl.seg.insert(pl.seg.end(), 64, i);
        }
        pl.total = 64 * pl.nseg;
        CHECK(bitmap_extent(pl.lpos.data(), 0, pl.nseg, pl.total).cn == 128, "128 segments of 64 fill the span exactly");
        for (int nsplit : {1, 3, 32})
            check_slices_and_bitmap(pl, nsplit, 256);
    }
    // an empty plan has only empty slices
    for (int nsplit : {1, 3, 32})
        for (int split = 0; split < nsplit; split++) {
            const ScanSlice sl = scan_slice(0, nsplit, split, 256);
            CHECK(sl.lo == 0 && sl.hi == 0, "empty plan: slice [%u, %u)", sl.lo, sl.hi);
        }
    if (failures)
        printf("%d checks failed\n", failures);
    else
        printf("scan_steps ok\n");
    return failures ? 1 : 0;
}
