// The arithmetic the in-place updates of the resident lists share (append 3.10, removal 3.11, Grouping append 3.12;
// DESIGN.md 1b): which list a row lies in, the source row a destination row takes, where a batch row goes, the 16-byte
// groups of a destination range and the copy of one of them, and the sizes of the workspace.  One copy; the device steps
// are in update_steps.h, the host cores (capi_update.cpp) size their buffers from here.  No HIP in here:
// tests/cpp/update_math_tool.cpp checks it on the host against plain serial loops, at a tile of 8 rows as well as of 2048.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFHNSW_UPDATE_FN __host__ __device__ __forceinline__
#define IVFHNSW_UPDATE_UNROLL _Pragma("unroll")
#else
#define IVFHNSW_UPDATE_FN inline
#define IVFHNSW_UPDATE_UNROLL
#endif

namespace ivfhnsw_gpu_impl {

constexpr uint32_t kSkip = 0xffffffffu; // a destination row with no old source row (a new code, or past the end): a hole

// ---- rows and lists.  The largest c in [lo, hi] with start[c] <= r (start[lo] <= r holds); among equal starts (empty
// lists) the last one, which is the list that holds the row.
template <class P> IVFHNSW_UPDATE_FN uint32_t list_of_row(P start, uint32_t lo, uint32_t hi, uint32_t r)
{
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (start[mid] <= r)
            lo = mid;
        else
            hi = mid - 1;
    }
    return lo;
}

// the old local row that row `off` of a list's new range takes: the list's old rows lead, the batch's follow (holes)
IVFHNSW_UPDATE_FN uint32_t list_source(uint32_t off, uint32_t old_len, uint32_t loff_c)
{
    return off < old_len ? loff_c + off : kSkip;
}

// the same for a Grouping list the batch touches: pn / po = the list's nsubc new / old exclusive prefix sums of sub-group
// sizes.  Every sub-group keeps its old rows in front of its new ones.
template <class P>
IVFHNSW_UPDATE_FN uint32_t grouping_source(P pn, P po, uint32_t nsubc, uint32_t off, uint32_t old_len, uint32_t loff_c)
{
    // the largest s with pn[s] <= off: the sub-group that holds row off (it is not empty, as the next prefix lies above)
    const uint32_t s = list_of_row(pn, 0u, nsubc - 1, off);
    const uint32_t within = off - pn[s];
    const uint32_t old_size = (s + 1 < nsubc ? po[s + 1] : old_len) - po[s];
    return within < old_size ? loff_c + po[s] + within : kSkip;
}

// prefix sums per table a Grouping tile keeps in LDS (16 lists at nsubc 64), and the words it loads for its lists
// lo .. hi: all of them, or none when they do not fit (the rows then search in global memory)
constexpr uint32_t kPrefixCache = 1024;
IVFHNSW_UPDATE_FN uint32_t prefix_cache_words(uint32_t lo, uint32_t hi, uint32_t nsubc)
{
    return (uint64_t)(hi - lo + 1) * nsubc <= kPrefixCache ? (hi - lo + 1) * nsubc : 0u;
}

// the new local row of row p of the batch sorted stably by list (IVFADC) or by (list, sub-group) (Grouping): nstart_c =
// the first sorted row of its list.  IVFADC: behind the list's old rows and the batch rows sorted before it.  Grouping:
// behind the old rows of the sub-groups up to its own (pre_old + size) and every batch row sorted before it in the list.
IVFHNSW_UPDATE_FN size_t append_dest_row(uint32_t lstart_c, uint32_t old_len, size_t p, uint32_t nstart_c)
{
    return (size_t)lstart_c + old_len + (p - nstart_c);
}
IVFHNSW_UPDATE_FN size_t grouping_dest_row(uint32_t lstart_c, uint32_t pre_old_cs, uint32_t size_cs, size_t p, uint32_t nstart_c)
{
    return (size_t)lstart_c + pre_old_cs + size_cs + (p - nstart_c);
}

// ---- the 16-byte groups of a destination range [d0, d0 + n) of elements (dwords; bytes for norm codes, four to a
// dword).  Group gi covers elements [4 gi - head, 4 gi - head + 4) of the range, counted from d0; the first and the last
// group may reach outside it, and what lies outside belongs to a neighbouring tile.  ALIGNED: d0 % 4 == 0 is known when
// the code is compiled (a destination tile of 2048 rows), so head is the constant 0 and no element lies in front of the
// range.  n < 2^31 (a tile's dwords), so an element index is an int32_t and "in the range" one unsigned comparison.
template <bool ALIGNED> IVFHNSW_UPDATE_FN uint32_t group_head(uint64_t d0) { return ALIGNED ? 0u : (uint32_t)(d0 & 3); }
IVFHNSW_UPDATE_FN uint32_t group_count(uint32_t head, uint32_t n) { return (head + n + 3) / 4; }
IVFHNSW_UPDATE_FN int32_t group_first(uint32_t gi, uint32_t head) { return (int32_t)(gi * 4 - head); }
template <bool ALIGNED> IVFHNSW_UPDATE_FN bool group_elem_front(int32_t e0, int u) { return !ALIGNED && e0 + u < 0; }
IVFHNSW_UPDATE_FN bool group_elem_in(int32_t e0, int u, uint32_t n) { return (uint32_t)(e0 + u) < n; }
template <bool ALIGNED> IVFHNSW_UPDATE_FN bool group_whole(int32_t e0, uint32_t n)
{
    return !group_elem_front<ALIGNED>(e0, 0) && (uint32_t)e0 + 4 <= n;
}

// element e of a range of rows of q dwords is dword k of row j; step() moves to the next element
struct GroupWalk {
    uint32_t j, k;
    IVFHNSW_UPDATE_FN GroupWalk(int32_t e0, uint32_t q)
    {
        const uint32_t ef = (uint32_t)(e0 < 0 ? 0 : e0); // elements in front of the range are not walked
        j = ef / q;
        k = ef - j * q;
    }
    IVFHNSW_UPDATE_FN void step(uint32_t q)
    {
        if (++k == q) {
            k = 0;
            j++;
        }
    }
};

// the fast path of a group, one 16-byte load: all four source rows sr[u] present and their dwords sr[u] * q + k[u]
// consecutive.  Inside a row they are; where the walk enters a row (k[u] == 0) it must be the one behind the row before.
IVFHNSW_UPDATE_FN bool group_is_run(const uint32_t sr[4], const uint32_t k[4])
{
    bool run = sr[0] != kSkip;
    IVFHNSW_UPDATE_UNROLL
    for (int u = 1; u < 4; u++)
        run = run && sr[u] != kSkip && (k[u] != 0 || sr[u] == sr[u - 1] + 1);
    return run;
}

// One group of the gathered dword copy: destination element e = j * q + k takes source dword s_src[j] * q + k, a hole
// (s_src[j] == kSkip) gives 0.  A whole group is one 16-byte store, of one 16-byte load when its sources are a run and of
// four dword loads otherwise; a group the range covers in part stores its own dwords only, so neighbouring tiles never
// write the same bytes.  m is the memory: load(s), load4(s, v), store(d, x), store4(d, v) with d counted from group 0.
template <bool ALIGNED, class M>
IVFHNSW_UPDATE_FN void copy_group_dwords(const M &m, const uint32_t *s_src, uint32_t gi, uint32_t head, uint32_t ndw, uint32_t q)
{
    const int32_t e0 = group_first(gi, head);
    GroupWalk w(e0, q);
    uint32_t sr[4], k[4];
    bool in[4];
    IVFHNSW_UPDATE_UNROLL
    for (int u = 0; u < 4; u++) {
        in[u] = group_elem_in(e0, u, ndw);
        sr[u] = in[u] ? s_src[w.j] : kSkip;
        k[u] = w.k;
        if (!group_elem_front<ALIGNED>(e0, u))
            w.step(q);
    }
    uint32_t v[4];
    if (group_is_run(sr, k)) {
        m.load4((size_t)sr[0] * q + k[0], v);
    } else {
        IVFHNSW_UPDATE_UNROLL
        for (int u = 0; u < 4; u++)
            v[u] = sr[u] != kSkip ? m.load((size_t)sr[u] * q + k[u]) : 0u;
    }
    if (group_whole<ALIGNED>(e0, ndw)) {
        m.store4((size_t)gi * 4, v);
    } else {
        IVFHNSW_UPDATE_UNROLL
        for (int u = 0; u < 4; u++)
            if (in[u])
                m.store((size_t)gi * 4 + u, v[u]);
    }
}

// The same at byte granularity (norm codes, one byte per row): a dword the range owns whole is one dword store of four
// gathered bytes, the range's two ends are byte stores.  m: load(s) a byte, store(d, byte), store4(d, dword).
template <bool ALIGNED, class M>
IVFHNSW_UPDATE_FN void copy_group_bytes(const M &m, const uint32_t *s_src, uint32_t gi, uint32_t head, uint32_t n)
{
    const int32_t e0 = group_first(gi, head);
    uint32_t w = 0;
    bool in[4];
    IVFHNSW_UPDATE_UNROLL
    for (int u = 0; u < 4; u++) {
        in[u] = group_elem_in(e0, u, n);
        const uint32_t sr = in[u] ? s_src[e0 + u] : kSkip;
        w |= (uint32_t)(sr != kSkip ? m.load(sr) : 0u) << (8 * u);
    }
    if (group_whole<ALIGNED>(e0, n)) {
        m.store4((size_t)gi * 4, w);
    } else {
        IVFHNSW_UPDATE_UNROLL
        for (int u = 0; u < 4; u++)
            if (in[u])
                m.store((size_t)gi * 4 + u, (uint8_t)(w >> (8 * u)));
    }
}

// ---- the removal mask: one bit per row, 64 rows to a word, a tile's words scanned by one wavefront.  The new place of
// kept row b of word w inside its tile: the tile's kept rows in front of the word, and the word's in front of the bit.
IVFHNSW_UPDATE_FN uint32_t kept_rank(uint32_t pre_w, unsigned long long kept, uint32_t b)
{
    return pre_w + (uint32_t)__builtin_popcountll(kept & ((1ull << b) - 1ull));
}

// ---- the upsert: a removal and an append in one rebuild.  rscan / nstart = the exclusive scans of the
// rows each list loses / gains, kscan = that of the rows each source tile keeps.  The new list c is its surviving old rows,
// in order, then its batch rows: it starts at start[c] - rscan[c] + nstart[c].
// The kept rows of a tile in front of its row x (0 <= x <= the tile's rows): pre / kept as the compaction holds them
// (words of 1 << wshift rows; 64 on the device), so kept row x has this rank inside the tile.
IVFHNSW_UPDATE_FN uint32_t kept_before(const uint32_t *pre, const unsigned long long *kept, uint32_t x, uint32_t wshift, uint32_t words)
{
    const uint32_t w = x >> wshift;
    return w >= words ? pre[words] : kept_rank(pre[w], kept[w], x & ((1u << wshift) - 1u));
}

// The piece of a source tile that lies in one list: from old row a (a < r_end, the tile's end) to the end of the list
// that holds a, or the tile's.  lo .. hi = the lists the search looks at (start[lo] <= a; hi = the list of the next
// tile's first row).  The kept rows of one segment are contiguous in the new arrays; between two segments lie the batch
// rows of the first one's list and whatever the lists in between gain.
struct TileSegment {
    uint32_t list, end;
};
template <class P, class G>
IVFHNSW_UPDATE_FN TileSegment tile_segment(P start, G goff, uint32_t lo, uint32_t hi, uint32_t a, uint32_t r_end)
{
    const uint32_t c = list_of_row(start, lo, hi, a);
    const uint64_t e = (uint64_t)start[c] + (uint64_t)(goff[c + 1] - goff[c]);
    return {c, e < r_end ? (uint32_t)e : r_end};
}

// the new local row of the kept row with rank j inside its source tile (kscan_t kept rows lie in tiles in front of it)
// and list c: every kept row in front of it stays in front, and so do the batch rows of the lists in front of c
IVFHNSW_UPDATE_FN size_t upsert_kept_dest(uint32_t kscan_t, uint32_t j, uint32_t nstart_c)
{
    return (size_t)kscan_t + j + nstart_c;
}
// the new start of list c, and the new local row of row p of the batch sorted stably by list: behind the list's kept rows
// and the batch rows sorted before it
IVFHNSW_UPDATE_FN uint32_t upsert_list_start(uint32_t start_c, uint32_t rscan_c, uint32_t nstart_c)
{
    return start_c - rscan_c + nstart_c;
}
IVFHNSW_UPDATE_FN size_t upsert_batch_dest(uint32_t start_c, uint32_t old_len, uint32_t rscan_c, uint32_t rscan_c1, size_t p,
                                           uint32_t nstart_c)
{
    return (size_t)upsert_list_start(start_c, rscan_c, nstart_c) + (old_len - (rscan_c1 - rscan_c)) + (p - nstart_c);
}

// ---- workspace sizes, in elements
constexpr int kScanChunk = 4096; // elements per workgroup of the three-phase scan (launch_append_tables, launch_scan_excl_u32)

IVFHNSW_UPDATE_FN size_t update_tiles(uint64_t n_local, size_t tile_rows) { return (size_t)((n_local + tile_rows - 1) / tile_rows); }
// tile_first of the merge: one word per tile and the closing one; sized before the tiles are counted, hence + 2
IVFHNSW_UPDATE_FN size_t append_tile_words(uint64_t n_local2, size_t tile_rows) { return (size_t)(n_local2 / tile_rows) + 2; }
// removal mask words: whole tiles (the compaction reads every word of its tile), one tile at least
IVFHNSW_UPDATE_FN size_t remove_mask_words(size_t ntiles, size_t tile_rows) { return (ntiles ? ntiles : 1) * ((tile_rows + 63) / 64); }
// words of the scan's partial sums: two arrays of len elements scanned side by side
IVFHNSW_UPDATE_FN size_t append_scan_parts(size_t len) { return 2 * ((len + kScanChunk - 1) / kScanChunk); }
// key bits of a radix sort over 0..top
IVFHNSW_UPDATE_FN int bits_of(size_t top)
{
    int b = 1;
    while (b < 32 && top >> b)
        b++;
    return b;
}

} // namespace ivfhnsw_gpu_impl
