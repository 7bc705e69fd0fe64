// The host arithmetic the brute-force MFMA sweeps share (knn_mfma_kernel, exact_mfma_kernel, exact_range_kernel;
// DESIGN.md 1b): how the columns are cut into splits, how many splits a call takes, the size of the range search's tile
// map, and the one dispatch on a row's length.  One copy; the device steps are in sweep_steps.h.  No HIP in here:
// tests/cpp/sweep_plan_tool.cpp checks it on the host against the formulas it replaced.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "scan_dispatch.h"

// the functions a sweep kernel calls as well (the split cut, the strip layout): the same text for both compilers
#ifdef __HIPCC__
#define SWEEP_HD __host__ __device__
#else
#define SWEEP_HD
#endif

namespace ivfhnsw_gpu_impl {

// Columns per split: equal shares rounded up to the 32 columns of a tile, never none (an empty store still gets a
// split, whose kernels find c_begin >= c_end and read nothing).
SWEEP_HD inline size_t sweep_cols_per_split(size_t nx, int nsplit)
{
    size_t cps = (nx + nsplit - 1) / nsplit;
    cps = (cps + 31) & ~(size_t)31;
    return cps ? cps : 32;
}

// Splits of a call whose workgroups own rows_per_block query rows each:
// enough workgroups for two per CU; a split never shorter than 4096 columns
inline int sweep_splits_for(size_t nq, size_t nx, int rows_per_block)
{
    const size_t rpb = (size_t)rows_per_block;
    const size_t row_blocks = (nq + rpb - 1) / rpb;
    size_t s = (512 + row_blocks - 1) / row_blocks;
    const size_t max_s = (nx + 4095) / 4096;
    s = s > max_s ? max_s : s;
    s = s < 1 ? 1 : s;
    return (int)(s > 64 ? 64 : s);
}

// Words of the range search's tile map per (32 queries, split): one bit per 2^map_shift tiles, 32 bits to a word.
inline int sweep_map_words(size_t nx, int nsplit, int map_shift)
{
    const size_t tiles = sweep_cols_per_split(nx, nsplit) / 32;
    const size_t bits = (tiles + ((size_t)1 << map_shift) - 1) >> map_shift;
    return (int)((bits + 31) / 32);
}

// ---- the exact sweeps under a base filter
// The column map of a sweep: Dense = column c is row c; Masked = the same columns, data = one pass bit per row, 32 to a
// word; Indirect = the columns are the entries of data, the passing row numbers ascending.
enum { kSweepColsDense = 0, kSweepColsMasked = 1, kSweepColsIndirect = 2 };
struct SweepCols {
    int form = kSweepColsDense;
    const uint32_t *data = nullptr;
};

// Pass words of a store of n rows: word w covers rows [32 w, 32 w + 32).
inline size_t sweep_pass_words(size_t n) { return (n + 31) / 32; }

// The pass word of tile t of a split that begins at column c_begin.  Splits begin at multiples of 32
// (sweep_cols_per_split), so the tile's 32 columns are exactly the word's 32 rows.
inline size_t sweep_tile_word(size_t c_begin, size_t t) { return (c_begin >> 5) + t; }

// Is the list of passing rows kept beside the pass words: when at most an eighth of the rows pass.  It is then at most
// n / 2 bytes, while the list of a deny filter with few labels would be 4 bytes per row of the store.
inline bool sweep_pass_list_kept(size_t npass, size_t n) { return npass <= n / 8; }

// The form a filtered sweep takes: Indirect when the list is kept, else Masked; opt (set_option "exact_filter_form")
// 0 / 1 forces Masked / Indirect, -1 is the rule.
inline int sweep_filter_form(size_t npass, size_t n, int opt)
{
    if (opt == 0)
        return kSweepColsMasked;
    if (opt == 1)
        return kSweepColsIndirect;
    return sweep_pass_list_kept(npass, n) ? kSweepColsIndirect : kSweepColsMasked;
}

// ---- base filter slots: the exact sweeps with a row set per query
// The columns [*c_begin, *c_end) of split `split` of nsplit over nx columns: what the sweep kernels compute from
// cols_per_split, as one function, because under a strip plan every strip cuts ITS OWN nx (an Indirect slot's columns are
// its list).  The cuts tile [0, nx) in whole tiles of 32; a split beyond the columns is empty at nx.
SWEEP_HD inline void sweep_split_cut(size_t nx, int nsplit, int split, size_t *c_begin, size_t *c_end)
{
    const size_t cps = sweep_cols_per_split(nx, nsplit);
    *c_begin = (size_t)split * cps < nx ? (size_t)split * cps : nx;
    *c_end = *c_begin + cps < nx ? *c_begin + cps : nx;
}

// What a strip sweeps, one entry per slot and one for "none" (kStripNone): the form, its words or rows, its columns.
// kSweepColsNothing: the slot is not set, or no row passes it -- its queries get no strip.
enum { kSweepColsNothing = 3 };
constexpr int kStripSlots = 32;               // = IVFHNSW_FILTER_SLOTS
constexpr int kStripNone = kStripSlots;       // the bucket and table entry of IVFHNSW_SLOT_NONE
constexpr int kStripInvalid = kStripSlots + 1; // the bucket of a byte that names nothing
constexpr int kStripBuckets = kStripSlots + 2;
struct StripCols {
    const uint32_t *data;
    uint32_t nx, form;
};

SWEEP_HD inline int sweep_strip_bucket(uint8_t byte) { return byte < kStripSlots ? byte : byte == 0xff ? kStripNone : kStripInvalid; }

// Strips of 32 queries, each of one bucket: at most this many for m queries.  Sum over the 33 buckets that get strips of
// ceil(c / 32) <= sum of floor(c / 32) + 33 <= m / 32 + 33.
SWEEP_HD inline size_t sweep_strip_bound(size_t m) { return m / 32 + 33; }

// The strips of a chunk from its counts per bucket.  Ordered by form -- Dense, Masked, Indirect -- so that the sweep of a
// form takes the contiguous range [range[form][0], range[form][1]); inside a form by bucket.  first[b]: the first strip of
// bucket b, ~0 where it gets none (no query, the invalid bucket, a form of kSweepColsNothing).
struct StripLayout {
    uint32_t first[kStripBuckets];
    uint32_t range[3][2];
    uint32_t nstrips;
};
SWEEP_HD inline void sweep_strip_layout(const uint32_t *counts, const uint32_t *forms, StripLayout *out)
{
    uint32_t s = 0;
    for (int b = 0; b < kStripBuckets; b++)
        out->first[b] = ~0u;
    for (uint32_t f = 0; f < 3; f++) {
        out->range[f][0] = s;
        for (int b = 0; b <= kStripNone; b++)
            if (forms[b] == f && counts[b]) {
                out->first[b] = s;
                s += (counts[b] + 31) / 32;
            }
        out->range[f][1] = s;
    }
    out->nstrips = s;
}

// The strip plan of one chunk in device memory, as the kernels take it.  hdr: counts per bucket, the cursors the scatter
// advances, the layout.  strip_slot [bound]: the table entry of every strip.  strip_rows [bound * 32]: per strip row the
// chunk's query it holds, -1 = padding.  map_strip0: the chunk's first strip in the call's tile map (range search).
struct StripHdr {
    uint32_t counts[kStripBuckets], cursor[kStripBuckets];
    StripLayout lay;
};
// A strip's entry comes from the slot table (table[strip_slot[strip]], base filter slots) or, under base tags (DESIGN.md
// 3.22), from an entry of its own (strip_cols[strip]): which of the two is the column map's to say (ColsStrips), at
// compile time.
struct StripPlan {
    const StripCols *table = nullptr;
    const StripHdr *hdr = nullptr;
    const uint8_t *strip_slot = nullptr;
    const int32_t *strip_rows = nullptr;
    uint32_t map_strip0 = 0;
    const StripCols *strip_cols = nullptr;
};
// bytes of a chunk's plan of `bound` strips: header, rows, slots (each part 16-byte aligned)
inline size_t sweep_strip_hdr_bytes() { return (sizeof(StripHdr) + 15) & ~(size_t)15; }
inline size_t sweep_strip_plan_bytes(size_t bound) { return sweep_strip_hdr_bytes() + bound * 32 * sizeof(int32_t) + ((bound + 15) & ~(size_t)15); }

// ---- base tags: the exact sweeps with a 16-bit tag per store row and per query
// queries per pass of the exact k-search, and the bytes its partial tables [nsplit][rows][k] may take
constexpr size_t kExactChunk = 16384;
constexpr size_t kExactPartBytes = (size_t)256 << 20;
constexpr uint32_t kTagNone = 0xffffu;  // = IVFHNSW_TAG_NONE
constexpr size_t kTagValues = 65536;    // tag_off has kTagValues + 1 entries: tag t's rows are [tag_off[t], tag_off[t + 1])

// Strips of 32 queries, each of one tag: at most this many for m queries on a store with tags_in_use tags.  A bucket is a
// tag with rows, or "none"; there are at most min(m, tags_in_use + 1) non-empty ones, and the sum over them of
// ceil(c / 32) <= sum of floor(c / 32) + their number <= m / 32 + min(m, tags_in_use + 1).
SWEEP_HD inline size_t sweep_tag_strip_bound(size_t m, size_t tags_in_use)
{
    const size_t buckets = tags_in_use + 1;
    return m / 32 + (m < buckets ? m : buckets);
}

// Queries per pass of a _tags k-search: the most, in multiples of 128 up to kExactChunk, whose partial tables over the
// PADDED rows stay within kExactPartBytes -- nsplit * bound(chunk) * 32 * k * 8 bytes.  At 128 it always fits (nsplit <= 64,
// k <= 100: 64 * 132 * 32 * 100 * 8 = 216 MB), so the answer is never below 128.
inline size_t sweep_tag_chunk(int nsplit, size_t k, size_t tags_in_use)
{
    const size_t per_strip = (size_t)nsplit * 32 * k * sizeof(uint64_t);
    size_t chunk = kExactChunk;
    while (chunk > 128 && per_strip * sweep_tag_strip_bound(chunk, tags_in_use) > kExactPartBytes)
        chunk -= 128;
    return chunk;
}

// What the holder keeps for the plan: rows = the tagged row numbers ordered by (tag, row), off [kTagValues + 1] their
// starts per tag, n = the rows of the store.  off null: no tag array, every row is untagged.
struct TagRows {
    const uint32_t *off = nullptr;
    const uint32_t *rows = nullptr;
    uint32_t n = 0;
};

// bytes of a chunk's tag plan of `bound` strips: header, rows, one entry per strip
inline size_t sweep_tag_plan_bytes(size_t bound) { return sweep_strip_hdr_bytes() + bound * 32 * sizeof(int32_t) + bound * sizeof(StripCols); }

// ---- base values: the exact sweeps with a uint32 value per store row and an interval per query
// The holder keeps ALL row numbers ordered by (value, row), a valueless row last at 0xffffffff, so the rows whose value
// lies in [lo, hi] are one window [*a, *b) of positions of that order: *a the first position whose value is >= lo, *b the
// first whose value is > hi -- n when hi is the largest value there is.  lo > hi is empty (0, 0).  value_at(i) = the value
// at position i of the n; two binary searches.  The rule is value_math.h's: lo <= v <= hi, unsigned, inclusive.
template <class V> SWEEP_HD inline void sweep_value_window(V value_at, uint32_t n, uint32_t lo, uint32_t hi, uint32_t *a, uint32_t *b)
{
    *a = *b = 0;
    if (lo > hi)
        return;
    uint32_t l = 0, h = n;
    while (l < h) {
        const uint32_t mid = l + ((h - l) >> 1);
        if (value_at(mid) < lo)
            l = mid + 1;
        else
            h = mid;
    }
    *a = l;
    h = n; // (the second search begins at *a: no position below it holds a value above hi >= lo)
    if (hi != 0xffffffffu)
        while (l < h) {
            const uint32_t mid = l + ((h - l) >> 1);
            if (value_at(mid) <= hi)
                l = mid + 1;
            else
                h = mid;
        }
    *b = h;
}

// Strips of 32 queries of a chunk of m: the queries whose window is the whole store fill ceil(f / 32) Dense strips, those
// with any other non-empty window, in the order of their windows' starts, ceil(w / 32) windowed ones; f + w <= m, so
// ceil(f / 32) + ceil(w / 32) <= (f + w) / 32 + 2 <= m / 32 + 2.
SWEEP_HD inline size_t sweep_value_strip_bound(size_t m) { return m / 32 + 2; }

// Queries per pass of a _values k-search: as the plain call's rule, over the padded rows of the strip bound --
// nsplit * bound(chunk) * 32 * k * 8 bytes within kExactPartBytes, in multiples of 128, never below 128
// (64 * 6 * 32 * 100 * 8 = 9.8 MB).
inline size_t sweep_value_chunk(int nsplit, size_t k)
{
    const size_t per_strip = (size_t)nsplit * 32 * k * sizeof(uint64_t);
    size_t chunk = kExactChunk;
    while (chunk > 128 && per_strip * sweep_value_strip_bound(chunk) > kExactPartBytes)
        chunk -= 128;
    return chunk;
}

// What the holder keeps for the plan: vals = the value of every row, rows = all row numbers ordered by (value, row),
// n = the rows of the store.  Null: no value array, every row is valueless.
struct ValueRows {
    const uint32_t *vals = nullptr;
    const uint32_t *rows = nullptr;
    uint32_t n = 0;
};
// a strip row's own window, relative to its strip's first column: the row counts columns [a, b) only; padding (0, 0)
struct StripWin {
    uint32_t a, b;
};

// bytes of a chunk's value plan of `bound` strips: a tag plan's, then a window per strip row
inline size_t sweep_value_plan_bytes(size_t bound) { return sweep_tag_plan_bytes(bound) + bound * 32 * sizeof(StripWin); }

// f(int_c<NS>()) for NS = ceil(d / 32) = 1 .. 8, the steps of 32 bytes a row of the uint8 store is read in (d <= 256)
template <class F> auto by_row_steps(int d, F &&f)
{
    switch ((d + 31) / 32) {
    case 1: return f(int_c<1>());
    case 2: return f(int_c<2>());
    case 3: return f(int_c<3>());
    case 4: return f(int_c<4>());
    case 5: return f(int_c<5>());
    case 6: return f(int_c<6>());
    case 7: return f(int_c<7>());
    default: return f(int_c<8>());
    }
}

} // namespace ivfhnsw_gpu_impl
