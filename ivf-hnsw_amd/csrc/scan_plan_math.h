// The index arithmetic every ADC scan kernel does on a query's plan: the slice of a workgroup, the segment of a position,
// the extent of a bitmap chunk.  One copy, shared by the kernels through scan_steps.h.  No HIP in here:
// tests/cpp/scan_steps_tool.cpp checks it on the host against a linear reference.
//
// A plan is nseg segments; lpos[i] is the position of segment i's first code in the query's flat array of `total`
// scored codes (ascending, no empty segments).  A staged chunk of cn segments is s_lpos[0 .. cn], s_lpos[cn] its end.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define IVFHNSW_SCAN_FN __host__ __device__ __forceinline__
#else
#define IVFHNSW_SCAN_FN inline
#endif

namespace ivfhnsw_gpu_impl {

IVFHNSW_SCAN_FN uint32_t scan_umin(uint32_t a, uint32_t b) { return a < b ? a : b; }

// Workgroup `split` of `nsplit` scores positions [lo, hi) of a query: equal shares rounded up to the block width
// (`threads`, a power of two), the last ones short or empty.
struct ScanSlice {
    uint32_t lo, hi;
};
IVFHNSW_SCAN_FN ScanSlice scan_slice(uint32_t total, int nsplit, int split, int threads)
{
    uint32_t per = (total + nsplit - 1) / nsplit;
    per = (per + (uint32_t)(threads - 1)) & ~(uint32_t)(threads - 1);
    const uint32_t lo = scan_umin((uint32_t)split * per, total);
    return ScanSlice{lo, scan_umin(lo + per, total)};
}

// Where the chunk of segments [cs, cs + cn) ends: at the next segment's start, or at the plan's end.
IVFHNSW_SCAN_FN uint32_t plan_chunk_end(const uint32_t *lpos, uint32_t cs, uint32_t cn, uint32_t nseg, uint32_t total)
{
    return (cs + cn == nseg) ? total : lpos[cs + cn];
}

// The segment of position p in a staged chunk: the first s with s_lpos[s + 1] > p, searched upward from the segment the
// lane was in before (positions only grow).  p < s_lpos[cn].  Three policies, one result:
// step by step -- plans of whole lists with at most 64 segments, where the next position is in this list or the next
struct SeekLinear {
    static IVFHNSW_SCAN_FN uint32_t seek(const uint32_t *s_lpos, uint32_t s, uint32_t, uint32_t p)
    {
        while (p >= s_lpos[s + 1])
            s++;
        return s;
    }
};
// by halves: the first s in [a, b] with s_lpos[s + 1] > p
IVFHNSW_SCAN_FN uint32_t seek_by_halves(const uint32_t *s_lpos, uint32_t a, uint32_t b, uint32_t p)
{
    while (a < b) {
        const uint32_t mid = (a + b) >> 1;
        if (s_lpos[mid + 1] > p)
            b = mid;
        else
            a = mid + 1;
    }
    return a;
}
struct SeekHalves {
    static IVFHNSW_SCAN_FN uint32_t seek(const uint32_t *s_lpos, uint32_t s, uint32_t cn, uint32_t p)
    {
        return seek_by_halves(s_lpos, s, cn - 1, p);
    }
};
// Inverted lists are about as long as a block's stride (1024 positions), so the segment is usually the next one or the
// one after: two steps forward, then by halves (which plans of sub-groups need).
struct SeekStep2Halves {
    static IVFHNSW_SCAN_FN uint32_t seek(const uint32_t *s_lpos, uint32_t s, uint32_t cn, uint32_t p)
    {
        uint32_t a = s, b = cn - 1;
        if (a < b && s_lpos[a + 1] <= p) {
            a++;
            if (a < b && s_lpos[a + 1] <= p)
                a++;
            else
                b = a;
        } else {
            b = a;
        }
        return seek_by_halves(s_lpos, a, b, p);
    }
};

// The first segment a slice touches: the last one starting at or before lo.
IVFHNSW_SCAN_FN uint32_t first_segment(const uint32_t *lpos, uint32_t nseg, uint32_t lo)
{
    uint32_t a = 0;
    if (lo > 0) {
        uint32_t b = nseg - 1;
        while (a < b) {
            const uint32_t mid = (a + b + 1) >> 1;
            if (lpos[mid] <= lo)
                a = mid;
            else
                b = mid - 1;
        }
    }
    return a;
}

// The bitmap form (plans of short segments) takes the plan in chunks of at most kBmSegCap segments spanning at most
// kBmSpanCap positions: one bit per position, set where a segment starts, plus the starts before every 64-position word.
constexpr int kBmSegCap = 256;
constexpr int kBmSpanCap = 8192;
constexpr int kBmSpanWords = kBmSpanCap / 64;

// The chunk that starts at segment cs: cn segments, positions [lpos[cs], ch).  As many segments as fit the plan buffer
// AND the span; one oversized segment goes alone (`single`: no bitmap, every position belongs to segment 0).
struct BitmapExtent {
    uint32_t cn, ch, nwords;
    bool single;
};
IVFHNSW_SCAN_FN BitmapExtent bitmap_extent(const uint32_t *lpos, uint32_t cs, uint32_t nseg, uint32_t total)
{
    const uint32_t cl = lpos[cs];
    uint32_t cn = scan_umin((uint32_t)kBmSegCap, nseg - cs);
    const uint32_t end_all = plan_chunk_end(lpos, cs, cn, nseg, total);
    if (end_all - cl > (uint32_t)kBmSpanCap) {
        uint32_t a = 1, b = cn > 1 ? cn - 1 : 1; // largest count whose end stays inside the span (or 1)
        while (a < b) {
            const uint32_t mid = (a + b + 1) >> 1;
            if (lpos[cs + mid] - cl <= (uint32_t)kBmSpanCap)
                a = mid;
            else
                b = mid - 1;
        }
        cn = a;
    }
    const uint32_t ch = plan_chunk_end(lpos, cs, cn, nseg, total);
    const bool single = ch - cl > (uint32_t)kBmSpanCap;
    return BitmapExtent{cn, ch, single ? 0u : (ch - cl + 63) >> 6, single};
}

// The chunk segment of the position at bit `lane` of bitmap word `mw`: `pref` starts before the word, `below` set bits of
// the word under the lane's (v_mbcnt on the device), and the lane's own bit if it starts one.
IVFHNSW_SCAN_FN uint32_t bitmap_segment(uint32_t pref, unsigned long long mw, uint32_t below, int lane)
{
    return pref + below + (uint32_t)((mw >> lane) & 1ull) - 1u;
}

} // namespace ivfhnsw_gpu_impl
