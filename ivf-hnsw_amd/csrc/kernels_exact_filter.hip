// The base filter of the exact calls (ivfhnsw_gpu_set_base_filter) in its two forms in HBM.
//   pass words   one bit per row of the store, 32 to a word (word w = rows [32 w, 32 w + 32), the 32 columns of a sweep
//                tile), bits at or beyond n zero: the label bitmap launch_remove_bits makes (kernels_remove.hip), cut or
//                zero-extended to n rows, with the mode folded in -- deny inverts it.
//   pass rows    the passing row numbers ascending, from the words: a popcount per word, the exclusive scan of the
//                counts (launch_scan_excl_u32) and a scatter in which every row finds its place by the bits below it.
// Below them the strip plan of a call with a base filter slot per query: count, layout, scatter.
// Then base tags: the holder's tag per row with the row lists per tag behind it (a stable sort of the row
// numbers by tag, launch_sort_by_key), and the strip plan of a call with a tag per query -- one bucket per tag among the
// chunk's queries, found with the same sort.
// Then base values: the holder's value per row with ALL row numbers ordered by (value, row) behind it (the
// same sort, 32 key bits), the window of an interval in that order, the strip plan of a call with an interval per query --
// whole-store windows in Dense strips, the others sorted by their start into strips that span their windows -- and the
// reorder of a range call's results to (query, label).
#include "ivfhnsw_kernels.h"
#include "device_common.h"

#include <algorithm>

namespace ivfhnsw_gpu_impl {

namespace {

// one thread per word; one atomic per wavefront for the count of passing rows
__global__ __launch_bounds__(256) void pass_words_kernel(const uint32_t *__restrict__ bits, size_t bit_words, uint64_t n,
                                                         size_t nwords, int deny, uint32_t *__restrict__ words,
                                                         unsigned long long *__restrict__ count)
{
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    uint32_t v = 0;
    if (w < nwords) {
        v = bits != nullptr && w < bit_words ? bits[w] : 0u;
        if (deny)
            v = ~v;
        const uint64_t left = n - (uint64_t)w * 32; // rows of the word inside the store: >= 1
        if (left < 32)
            v &= (1u << left) - 1u;
        words[w] = v;
    }
    uint32_t c = (uint32_t)__popc(v);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1)
        c += __shfl_xor(c, o);
    if ((threadIdx.x & 63) == 0 && c)
        atomicAdd(count, (unsigned long long)c);
}

// cnt [nwords + 1]: the passing rows of every word, slot nwords zero (its scan is the total)
__global__ __launch_bounds__(256) void pass_counts_kernel(const uint32_t *__restrict__ words, size_t nwords, uint32_t *__restrict__ cnt)
{
    const size_t w = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (w <= nwords)
        cnt[w] = w < nwords ? (uint32_t)__popc(words[w]) : 0u;
}

// one thread per row: a passing row goes to pre[its word] + the passing rows below it in the word
__global__ __launch_bounds__(256) void pass_rows_kernel(const uint32_t *__restrict__ words, uint64_t n, const uint32_t *__restrict__ pre,
                                                        uint32_t *__restrict__ rows)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r >= n)
        return;
    const uint32_t v = words[r >> 5], b = (uint32_t)(r & 31);
    if ((v >> b) & 1u)
        rows[pre[r >> 5] + (uint32_t)__popc(v & ((1u << b) - 1u))] = (uint32_t)r;
}

// ---- base filter slots: the strip plan of one chunk of an exact _slots call --------------------------
// the bucket a query is counted in: its byte's, or the invalid one when the byte's table entry sweeps nothing (a slot that
// is not set, or that no row passes)
__device__ __forceinline__ int strip_query_bucket(const StripCols *__restrict__ table, uint8_t byte)
{
    const int b = sweep_strip_bucket(byte);
    return b != kStripInvalid && table[b].form == kSweepColsNothing ? kStripInvalid : b;
}

// hdr->counts: the chunk's queries per bucket (hdr zeroed before); a histogram per workgroup in LDS first
__global__ __launch_bounds__(256) void strip_count_kernel(const uint8_t *__restrict__ slots, size_t m, const StripCols *__restrict__ table,
                                                          StripHdr *__restrict__ hdr)
{
    __shared__ uint32_t s_cnt[kStripBuckets];
    if (threadIdx.x < kStripBuckets)
        s_cnt[threadIdx.x] = 0;
    __syncthreads();
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < m)
        atomicAdd(&s_cnt[strip_query_bucket(table, slots[q])], 1u);
    __syncthreads();
    if (threadIdx.x < kStripBuckets && s_cnt[threadIdx.x])
        atomicAdd(&hdr->counts[threadIdx.x], s_cnt[threadIdx.x]);
}

// one wavefront: the layout from the counts (sweep_strip_layout), then the table entry of every strip
__global__ __launch_bounds__(64) void strip_layout_kernel(const StripCols *__restrict__ table, StripHdr *__restrict__ hdr,
                                                          uint8_t *__restrict__ strip_slot, uint32_t bound)
{
    __shared__ StripLayout s_lay;
    if (threadIdx.x == 0) {
        uint32_t forms[kStripNone + 1];
        for (int b = 0; b <= kStripNone; b++)
            forms[b] = table[b].form;
        sweep_strip_layout(hdr->counts, forms, &s_lay);
        hdr->lay = s_lay;
    }
    __syncthreads();
    for (int b = 0; b <= kStripNone; b++) {
        const uint32_t first = s_lay.first[b], n = (hdr->counts[b] + 31) / 32;
        if (first == ~0u)
            continue;
        for (uint32_t i = threadIdx.x; i < n; i += 64)
            if (first + i < bound) // (always: sweep_strip_bound)
                strip_slot[first + i] = (uint8_t)b;
    }
}

// every query of a bucket with strips takes the next row of its bucket's strips (strip_rows filled with -1 before); the
// order inside a bucket is whichever the cursor gives: no result depends on it
__global__ __launch_bounds__(256) void strip_scatter_kernel(const uint8_t *__restrict__ slots, size_t m, const StripCols *__restrict__ table,
                                                            StripHdr *__restrict__ hdr, int32_t *__restrict__ strip_rows)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m)
        return;
    const int b = strip_query_bucket(table, slots[q]);
    const uint32_t first = hdr->lay.first[b];
    if (first == ~0u)
        return;
    const uint32_t pos = atomicAdd(&hdr->cursor[b], 1u);
    if (pos < hdr->counts[b]) // (always, unless the caller rewrote the bytes between the two passes)
        strip_rows[(size_t)first * 32 + pos] = (int32_t)q;
}

// ---- base tags: the holder's arrays -------------------------------------------------------------------
// tags[rows[i]] = vals[i] for the rows inside the store (a row number >= n matches nothing).  Two entries share a 32-bit
// word; a 16-bit store touches its own half only (as tags_scatter_kernel, kernels_filter.hip).
__global__ __launch_bounds__(256) void base_tags_scatter_kernel(const uint32_t *__restrict__ rows, const uint16_t *__restrict__ vals,
                                                                size_t cnt, uint64_t n, uint16_t *__restrict__ tags)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += stride)
        if (rows[i] < n)
            tags[rows[i]] = vals[i];
}

// ... and the check behind it: a row given two different tags kept one of them, so the other entry does not read back
__global__ __launch_bounds__(256) void base_tags_verify_kernel(const uint32_t *__restrict__ rows, const uint16_t *__restrict__ vals,
                                                               size_t cnt, uint64_t n, const uint16_t *__restrict__ tags,
                                                               uint32_t *__restrict__ conflict)
{
    const size_t stride = (size_t)gridDim.x * 256;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += stride)
        bad |= rows[i] < n && tags[rows[i]] != vals[i];
    if (bad)
        atomicOr(conflict, 1u);
}

// the sort's keys: a row's tag as 32 bits
__global__ __launch_bounds__(256) void base_tags_keys_kernel(const uint16_t *__restrict__ tags, uint64_t n, uint32_t *__restrict__ keys)
{
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (r < n)
        keys[r] = tags[r];
}

// off[t] = the rows whose tag is below t, t = 0 .. kTagValues: the first place of the rows sorted by tag whose tag is not
// below t (a binary search per thread).  Tag t's rows are sorted [off[t], off[t + 1]); off[kTagNone] = the tagged rows.
__global__ __launch_bounds__(256) void base_tags_offsets_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ sorted,
                                                                uint32_t n, uint32_t *__restrict__ off)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t > kTagValues)
        return;
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[sorted[mid]] < t)
            lo = mid + 1;
        else
            hi = mid;
    }
    off[t] = lo;
}

// stats (zeroed before): [0] = the tags that have rows, [1] = the most rows of one tag
__global__ __launch_bounds__(256) void base_tags_stats_kernel(const uint32_t *__restrict__ off, uint32_t *__restrict__ stats)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    const uint32_t c = t < kTagNone ? off[t + 1] - off[t] : 0u;
    const uint32_t used = (uint32_t)__popcll(__ballot(c != 0));
    if ((threadIdx.x & 63) == 0 && used)
        atomicAdd(&stats[0], used);
    if (c)
        atomicMax(&stats[1], c);
}

// ---- base tags: the strip plan of one chunk of an exact _tags call ----------------------------------------------------
// A query's bucket: 0 for "none" -- so that its strips, the Dense ones, come first -- else its tag + 1.
__device__ __forceinline__ uint32_t tag_bucket(uint16_t tag) { return ((uint32_t)tag + 1u) & 0xffffu; }

// keys[q] = the bucket of query q; qcnt[bucket] (zeroed before) counts them
__global__ __launch_bounds__(256) void tag_query_keys_kernel(const uint16_t *__restrict__ qtags, size_t m, uint32_t *__restrict__ keys,
                                                             uint32_t *__restrict__ qcnt)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m)
        return;
    const uint32_t b = tag_bucket(qtags[q]);
    keys[q] = b;
    atomicAdd(&qcnt[b], 1u);
}

// nstr[b] = the strips of bucket b, b = 0 .. kTagValues (the last: none, the scan's total): ceil(queries / 32) where the
// bucket sweeps something -- "none" the store, a tag its rows -- else 0, its queries keep the padding
__global__ __launch_bounds__(256) void tag_bucket_strips_kernel(const uint32_t *__restrict__ qcnt, TagRows tr, uint32_t *__restrict__ nstr)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b > kTagValues)
        return;
    uint32_t s = 0;
    if (b < kTagValues && qcnt[b]) {
        const bool rows = b == 0 ? tr.n != 0 : tr.off != nullptr && tr.off[b] > tr.off[b - 1];
        s = rows ? (qcnt[b] + 31) / 32 : 0u;
    }
    nstr[b] = s;
}

// Query sorted[i], the i-th of the chunk's queries in the stable order by bucket, takes row (i - qoff[b]) of its bucket's
// strips (strip_rows filled with -1 before); the query in a strip's row 0 writes the strip's entry, the first thread the
// layout.  qoff / sfirst: the exclusive scans of qcnt / nstr.
__global__ __launch_bounds__(256) void tag_scatter_kernel(const uint32_t *__restrict__ sorted, const uint32_t *__restrict__ keys, size_t m,
                                                          const uint32_t *__restrict__ qoff, const uint32_t *__restrict__ sfirst, TagRows tr,
                                                          uint32_t bound, StripHdr *__restrict__ hdr, int32_t *__restrict__ strip_rows,
                                                          StripCols *__restrict__ strip_cols)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i == 0) {
        const uint32_t dense = min(sfirst[1], bound), all = min(sfirst[kTagValues], bound); // (never above: sweep_tag_strip_bound)
        hdr->lay.range[kSweepColsDense][0] = 0;
        hdr->lay.range[kSweepColsDense][1] = dense;
        hdr->lay.range[kSweepColsMasked][0] = hdr->lay.range[kSweepColsMasked][1] = dense;
        hdr->lay.range[kSweepColsIndirect][0] = dense;
        hdr->lay.range[kSweepColsIndirect][1] = all;
        hdr->lay.nstrips = all;
    }
    if (i >= m)
        return;
    const uint32_t q = sorted[i], b = keys[q];
    const uint32_t first = sfirst[b], pos = (uint32_t)i - qoff[b];
    if (sfirst[b + 1] == first)
        return;
    const uint32_t strip = first + (pos >> 5);
    if (strip >= bound)
        return;
    strip_rows[(size_t)strip * 32 + (pos & 31)] = (int32_t)q;
    if ((pos & 31) == 0) {
        StripCols e;
        if (b == 0)
            e = {nullptr, tr.n, (uint32_t)kSweepColsDense};
        else
            e = {tr.rows + tr.off[b - 1], tr.off[b] - tr.off[b - 1], (uint32_t)kSweepColsIndirect};
        strip_cols[strip] = e;
    }
}

// ---- base values: the holder's arrays -----------------------------------------------------------------
// vals[rows[i]] = v[i] for the rows inside the store, and the check behind it, as the tags' pair above
__global__ __launch_bounds__(256) void base_values_scatter_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ v,
                                                                  size_t cnt, uint64_t n, uint32_t *__restrict__ vals)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += stride)
        if (rows[i] < n)
            vals[rows[i]] = v[i];
}

__global__ __launch_bounds__(256) void base_values_verify_kernel(const uint32_t *__restrict__ rows, const uint32_t *__restrict__ v,
                                                                 size_t cnt, uint64_t n, const uint32_t *__restrict__ vals,
                                                                 uint32_t *__restrict__ conflict)
{
    const size_t stride = (size_t)gridDim.x * 256;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < cnt; i += stride)
        bad |= rows[i] < n && vals[rows[i]] != v[i];
    if (bad)
        atomicOr(conflict, 1u);
}

// the window of the interval (lo, hi) in the holder's row order; without a value array every row holds 0xffffffff
__device__ __forceinline__ StripWin value_window(const ValueRows &vr, uint32_t lo, uint32_t hi)
{
    StripWin w;
    sweep_value_window([&](uint32_t i) { return vr.vals ? vr.vals[vr.rows[i]] : 0xffffffffu; }, vr.n, lo, hi, &w.a, &w.b);
    return w;
}

__global__ __launch_bounds__(256) void value_windows_kernel(const uint32_t *__restrict__ qr, size_t m, ValueRows vr, StripWin *__restrict__ win)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q < m)
        win[q] = value_window(vr, qr[2 * q], qr[2 * q + 1]);
}

// ---- base values: the strip plan of one chunk of an exact _values call --------------------------------------------------
// wabs[q] = the window of query q; keys[q] = what the chunk's queries are sorted by: 0 for a window that is the whole store
// -- its strips, the Dense ones, come first --, the window's start + 1 (<= n < 2^32 - 1) for any other that holds a row,
// 0xffffffff for an empty one, which gets no strip.  cnt (zeroed before): [0] the whole-store queries, [1] the windowed ones.
__global__ __launch_bounds__(256) void value_query_keys_kernel(const uint32_t *__restrict__ qr, size_t m, ValueRows vr,
                                                               StripWin *__restrict__ wabs, uint32_t *__restrict__ keys,
                                                               uint32_t *__restrict__ cnt)
{
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= m)
        return;
    const StripWin w = value_window(vr, qr[2 * q], qr[2 * q + 1]);
    wabs[q] = w;
    const bool none = w.a >= w.b, full = !none && w.a == 0 && w.b == vr.n;
    keys[q] = none ? 0xffffffffu : full ? 0u : w.a + 1u;
    if (!none)
        atomicAdd(&cnt[full ? 0 : 1], 1u);
}

// Query sorted[i], the i-th of the chunk's queries in the stable order by key, takes the next row of the Dense strips
// (i < cnt[0]) or of the windowed ones (strip_rows filled with -1, strip_win with empty windows before).  A windowed strip
// spans [A, B): A the start of its first query's window, the smallest of the strip, B the furthest end among its rows,
// which the thread of the strip's row 0 finds; a row's own window is kept relative to A.  The first thread writes the layout.
__global__ __launch_bounds__(256) void value_scatter_kernel(const uint32_t *__restrict__ sorted, const StripWin *__restrict__ wabs, size_t m,
                                                            const uint32_t *__restrict__ cnt, ValueRows vr, uint32_t bound,
                                                            StripHdr *__restrict__ hdr, int32_t *__restrict__ strip_rows,
                                                            StripCols *__restrict__ strip_cols, StripWin *__restrict__ strip_win)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    const uint32_t nfull = cnt[0], nwin = cnt[1];
    const uint32_t dense = min((nfull + 31) / 32, bound), all = min(dense + (nwin + 31) / 32, bound); // (never above: sweep_value_strip_bound)
    if (i == 0) {
        hdr->lay.range[kSweepColsDense][0] = 0;
        hdr->lay.range[kSweepColsDense][1] = dense;
        hdr->lay.range[kSweepColsMasked][0] = hdr->lay.range[kSweepColsMasked][1] = dense;
        hdr->lay.range[kSweepColsIndirect][0] = dense;
        hdr->lay.range[kSweepColsIndirect][1] = all;
        hdr->lay.nstrips = all;
    }
    if (i >= m || i >= (size_t)nfull + nwin)
        return;
    const uint32_t q = sorted[i];
    if (i < nfull) {
        const uint32_t strip = (uint32_t)i >> 5;
        if (strip >= dense)
            return;
        strip_rows[(size_t)strip * 32 + (i & 31)] = (int32_t)q;
        if ((i & 31) == 0)
            strip_cols[strip] = {nullptr, vr.n, (uint32_t)kSweepColsDense};
        return;
    }
    const uint32_t j = (uint32_t)i - nfull, strip = dense + (j >> 5);
    if (strip >= all)
        return;
    const uint32_t j0 = nfull + (j & ~31u), j1 = min(j0 + 32u, nfull + nwin);
    const uint32_t A = wabs[sorted[j0]].a;
    const StripWin w = wabs[q];
    strip_rows[(size_t)strip * 32 + (j & 31)] = (int32_t)q;
    strip_win[(size_t)strip * 32 + (j & 31)] = {w.a - A, w.b - A};
    if ((j & 31) == 0) {
        uint32_t B = w.b;
        for (uint32_t t = j0 + 1; t < j1; t++)
            B = max(B, wabs[sorted[t]].b);
        strip_cols[strip] = {vr.rows + A, B - A, (uint32_t)kSweepColsIndirect};
    }
}

// ---- base values: the results of a range call in label order -------------------------------------------------------------
// keys of result i: the low word of its label (row numbers are below 2^32), and the query whose results [lims[q],
// lims[q + 1]) hold place i
__global__ __launch_bounds__(256) void range_label_keys_kernel(const long long *__restrict__ labels, const uint64_t *__restrict__ lims,
                                                               uint32_t nq, size_t tot, uint32_t *__restrict__ klab, uint32_t *__restrict__ kq)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= tot)
        return;
    klab[i] = (uint32_t)labels[i];
    uint32_t lo = 0, hi = nq; // the last q with lims[q] <= i
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (lims[mid] <= i)
            lo = mid;
        else
            hi = mid;
    }
    kq[i] = lo;
}

__global__ __launch_bounds__(256) void range_gather_kernel(const uint32_t *__restrict__ order, size_t tot, const float *__restrict__ dist,
                                                           const long long *__restrict__ labels, float *__restrict__ out_d,
                                                           long long *__restrict__ out_l)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= tot)
        return;
    const uint32_t src = order[i];
    out_d[i] = dist[src];
    out_l[i] = labels[src];
}

} // namespace

hipError_t launch_base_values_apply(hipStream_t s, const uint32_t *rows, const uint32_t *v, size_t cnt, uint64_t n, uint32_t *vals,
                                    uint32_t *conflict)
{
    if (hipError_t e = hipMemsetAsync(conflict, 0, sizeof(uint32_t), s); e != hipSuccess)
        return e;
    if (cnt == 0)
        return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((cnt + 255) / 256, (size_t)1 << 16);
    hipLaunchKernelGGL(base_values_scatter_kernel, dim3(grid), dim3(256), 0, s, rows, v, cnt, n, vals);
    hipLaunchKernelGGL(base_values_verify_kernel, dim3(grid), dim3(256), 0, s, rows, v, cnt, n, vals, conflict);
    return hipGetLastError();
}

// 32 key bits from the identity: equal values keep ascending row
hipError_t launch_base_values_index(hipStream_t s, const uint32_t *vals, uint64_t n, uint32_t *ids_a, uint32_t *ids_b, uint32_t *hist,
                                    uint32_t **sorted)
{
    if (n == 0 || n >= 0xffffffffull)
        return hipErrorInvalidValue;
    return launch_sort_by_key(s, vals, n, 32, ids_a, ids_b, hist, sorted);
}

hipError_t launch_value_windows(hipStream_t s, const uint32_t *d_ranges, size_t m, const ValueRows &vr, StripWin *win)
{
    if (m == 0)
        return hipSuccess;
    if (!d_ranges || !win || (vr.vals && !vr.rows))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(value_windows_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s, d_ranges, m, vr, win);
    return hipGetLastError();
}

// keys, the sort's two permutations and its histograms; the windows; the two counts (padded to four words)
size_t value_plan_work_words(size_t m) { return 3 * m + 256 * ((m + kKmeansTile - 1) / kKmeansTile) + 2 * m + 4; }

hipError_t launch_value_strip_plan(hipStream_t s, const uint32_t *d_ranges, size_t m, const ValueRows &vr, void *plan, size_t bound,
                                   uint32_t *work, StripPlan *sp, const StripWin **win)
{
    if (m == 0 || m > kExactChunk || bound < sweep_value_strip_bound(m) || bound > 0x7fffffffull / 32 || !d_ranges || !plan || !work ||
        (vr.vals && !vr.rows))
        return hipErrorInvalidValue;
    StripHdr *hdr = reinterpret_cast<StripHdr *>(plan);
    int32_t *rows = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(plan) + sweep_strip_hdr_bytes());
    StripCols *cols = reinterpret_cast<StripCols *>(rows + bound * 32);
    StripWin *swin = reinterpret_cast<StripWin *>(cols + bound);
    uint32_t *keys = work, *ids_a = keys + m, *ids_b = ids_a + m, *hist = ids_b + m;
    uint32_t *cnt = hist + 256 * ((m + kKmeansTile - 1) / kKmeansTile);
    StripWin *wabs = reinterpret_cast<StripWin *>(cnt + 4);
    if (hipError_t e = hipMemsetAsync(hdr, 0, sweep_strip_hdr_bytes(), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(rows, 0xff, bound * 32 * sizeof(int32_t), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(cols, 0, bound * sizeof(StripCols) + bound * 32 * sizeof(StripWin), s); e != hipSuccess)
        return e; // (Dense over no column; every window empty)
    if (hipError_t e = hipMemsetAsync(cnt, 0, 4 * sizeof(uint32_t), s); e != hipSuccess)
        return e;
    const dim3 grid((unsigned)((m + 255) / 256));
    hipLaunchKernelGGL(value_query_keys_kernel, grid, dim3(256), 0, s, d_ranges, m, vr, wabs, keys, cnt);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    uint32_t *sorted = nullptr;
    if (hipError_t e = launch_sort_by_key(s, keys, m, 32, ids_a, ids_b, hist, &sorted); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(value_scatter_kernel, grid, dim3(256), 0, s, sorted, wabs, m, cnt, vr, (uint32_t)bound, hdr, rows, cols, swin);
    sp->table = nullptr;
    sp->hdr = hdr;
    sp->strip_slot = nullptr;
    sp->strip_rows = rows;
    sp->strip_cols = cols;
    *win = swin;
    return hipGetLastError();
}

// the label keys and the query keys, the sort's two permutations and its histograms
size_t range_by_label_work_words(size_t tot) { return 4 * tot + 256 * ((tot + kKmeansTile - 1) / kKmeansTile); }

hipError_t launch_range_by_label(hipStream_t s, const uint64_t *d_lims, size_t nq, size_t tot, const float *dist, const int64_t *labels,
                                 float *out_d, int64_t *out_l, uint32_t *work)
{
    if (tot == 0)
        return hipSuccess;
    if (nq == 0 || nq > 0x7fffffffull || tot >= 0xffffffffull || !d_lims || !dist || !labels || !out_d || !out_l || !work)
        return hipErrorInvalidValue;
    uint32_t *klab = work, *kq = klab + tot, *ids_a = kq + tot, *ids_b = ids_a + tot, *hist = ids_b + tot;
    const dim3 grid((unsigned)((tot + 255) / 256));
    const long long *lab = reinterpret_cast<const long long *>(labels);
    hipLaunchKernelGGL(range_label_keys_kernel, grid, dim3(256), 0, s, lab, d_lims, (uint32_t)nq, tot, klab, kq);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    // stable by the label, then from that order stable by the query: (query, label)
    uint32_t *order = nullptr;
    if (hipError_t e = launch_sort_by_key(s, klab, tot, 32, ids_a, ids_b, hist, &order); e != hipSuccess)
        return e;
    int qbits = 1;
    while (qbits < 32 && ((size_t)1 << qbits) < nq)
        qbits++;
    if (hipError_t e = launch_sort_by_key_from(s, kq, tot, qbits, order, ids_a, ids_b, hist, &order); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(range_gather_kernel, grid, dim3(256), 0, s, order, tot, dist, lab, out_d, reinterpret_cast<long long *>(out_l));
    return hipGetLastError();
}

hipError_t launch_base_tags_apply(hipStream_t s, const uint32_t *rows, const uint16_t *vals, size_t cnt, uint64_t n, uint16_t *tags,
                                  uint32_t *conflict)
{
    if (hipError_t e = hipMemsetAsync(conflict, 0, sizeof(uint32_t), s); e != hipSuccess)
        return e;
    if (cnt == 0)
        return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((cnt + 255) / 256, (size_t)1 << 16);
    hipLaunchKernelGGL(base_tags_scatter_kernel, dim3(grid), dim3(256), 0, s, rows, vals, cnt, n, tags);
    hipLaunchKernelGGL(base_tags_verify_kernel, dim3(grid), dim3(256), 0, s, rows, vals, cnt, n, tags, conflict);
    return hipGetLastError();
}

hipError_t launch_base_tags_index(hipStream_t s, const uint16_t *tags, uint64_t n, uint32_t *keys, uint32_t *ids_a, uint32_t *ids_b,
                                  uint32_t *hist, uint32_t *off, uint32_t *stats, uint32_t **sorted)
{
    if (n == 0 || n >= 0xffffffffull)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(base_tags_keys_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, tags, n, keys);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (hipError_t e = launch_sort_by_key(s, keys, n, 16, ids_a, ids_b, hist, sorted); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(stats, 0, 2 * sizeof(uint32_t), s); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(base_tags_offsets_kernel, dim3((unsigned)(kTagValues / 256 + 1)), dim3(256), 0, s, keys, *sorted, (uint32_t)n, off);
    hipLaunchKernelGGL(base_tags_stats_kernel, dim3((unsigned)(kTagValues / 256)), dim3(256), 0, s, off, stats);
    return hipGetLastError();
}

size_t tag_plan_work_words(size_t m)
{
    return 3 * m + 256 * ((m + kKmeansTile - 1) / kKmeansTile) + 2 * (kTagValues + 1) + append_scan_parts(kTagValues + 1);
}

hipError_t launch_tag_strip_plan(hipStream_t s, const uint16_t *d_tags, size_t m, const TagRows &tr, void *plan, size_t bound,
                                 uint32_t *work, StripPlan *sp)
{
    if (m == 0 || m > kExactChunk || bound < m / 32 + 1 || bound > 0x7fffffffull / 32 || !d_tags || !plan || !work)
        return hipErrorInvalidValue;
    StripHdr *hdr = reinterpret_cast<StripHdr *>(plan);
    int32_t *rows = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(plan) + sweep_strip_hdr_bytes());
    StripCols *cols = reinterpret_cast<StripCols *>(rows + bound * 32);
    uint32_t *keys = work, *ids_a = keys + m, *ids_b = ids_a + m, *hist = ids_b + m;
    uint32_t *qcnt = hist + 256 * ((m + kKmeansTile - 1) / kKmeansTile), *nstr = qcnt + kTagValues + 1, *part = nstr + kTagValues + 1;
    if (hipError_t e = hipMemsetAsync(hdr, 0, sweep_strip_hdr_bytes(), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(rows, 0xff, bound * 32 * sizeof(int32_t), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(cols, 0, bound * sizeof(StripCols), s); e != hipSuccess) // (Dense over no column)
        return e;
    if (hipError_t e = hipMemsetAsync(qcnt, 0, (kTagValues + 1) * sizeof(uint32_t), s); e != hipSuccess)
        return e;
    const dim3 grid((unsigned)((m + 255) / 256)), tgrid((unsigned)(kTagValues / 256 + 1));
    hipLaunchKernelGGL(tag_query_keys_kernel, grid, dim3(256), 0, s, d_tags, m, keys, qcnt);
    hipLaunchKernelGGL(tag_bucket_strips_kernel, tgrid, dim3(256), 0, s, qcnt, tr, nstr);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    uint32_t *sorted = nullptr;
    if (hipError_t e = launch_sort_by_key(s, keys, m, 16, ids_a, ids_b, hist, &sorted); e != hipSuccess)
        return e;
    if (hipError_t e = launch_scan_excl_u32(s, qcnt, kTagValues + 1, part); e != hipSuccess)
        return e;
    if (hipError_t e = launch_scan_excl_u32(s, nstr, kTagValues + 1, part); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(tag_scatter_kernel, grid, dim3(256), 0, s, sorted, keys, m, qcnt, nstr, tr, (uint32_t)bound, hdr, rows, cols);
    sp->table = nullptr;
    sp->hdr = hdr;
    sp->strip_slot = nullptr;
    sp->strip_rows = rows;
    sp->strip_cols = cols;
    return hipGetLastError();
}

hipError_t launch_strip_plan(hipStream_t s, const uint8_t *d_slots, size_t m, const StripCols *table, void *plan, size_t bound,
                             StripPlan *sp)
{
    if (m == 0 || m > 0x7fffffffull || bound < sweep_strip_bound(m) || !d_slots || !table || !plan)
        return hipErrorInvalidValue;
    StripHdr *hdr = reinterpret_cast<StripHdr *>(plan);
    int32_t *rows = reinterpret_cast<int32_t *>(static_cast<unsigned char *>(plan) + sweep_strip_hdr_bytes());
    uint8_t *slot = reinterpret_cast<uint8_t *>(rows + bound * 32);
    if (hipError_t e = hipMemsetAsync(hdr, 0, sweep_strip_hdr_bytes(), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(rows, 0xff, bound * 32 * sizeof(int32_t), s); e != hipSuccess)
        return e;
    if (hipError_t e = hipMemsetAsync(slot, kStripNone, bound, s); e != hipSuccess)
        return e;
    const dim3 grid((unsigned)((m + 255) / 256));
    hipLaunchKernelGGL(strip_count_kernel, grid, dim3(256), 0, s, d_slots, m, table, hdr);
    hipLaunchKernelGGL(strip_layout_kernel, dim3(1), dim3(64), 0, s, table, hdr, slot, (uint32_t)bound);
    hipLaunchKernelGGL(strip_scatter_kernel, grid, dim3(256), 0, s, d_slots, m, table, hdr, rows);
    sp->table = table;
    sp->hdr = hdr;
    sp->strip_slot = slot;
    sp->strip_rows = rows;
    return hipGetLastError();
}

hipError_t launch_pass_words(hipStream_t s, const uint32_t *bits, size_t bit_words, uint64_t n, int deny, uint32_t *words,
                             unsigned long long *count)
{
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), s); e != hipSuccess)
        return e;
    if (n == 0)
        return hipSuccess;
    if (n >= 0xffffffffull)
        return hipErrorInvalidValue;
    const size_t nwords = sweep_pass_words(n);
    hipLaunchKernelGGL(pass_words_kernel, dim3((unsigned)((nwords + 255) / 256)), dim3(256), 0, s, bits, bit_words, n, nwords, deny,
                       words, count);
    return hipGetLastError();
}

hipError_t launch_pass_rows(hipStream_t s, const uint32_t *words, uint64_t n, uint32_t *cnt, uint32_t *part, uint32_t *rows)
{
    if (n == 0)
        return hipSuccess;
    if (n >= 0xffffffffull)
        return hipErrorInvalidValue;
    const size_t nwords = sweep_pass_words(n);
    hipLaunchKernelGGL(pass_counts_kernel, dim3((unsigned)((nwords + 256) / 256)), dim3(256), 0, s, words, nwords, cnt);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    if (hipError_t e = launch_scan_excl_u32(s, cnt, nwords + 1, part); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(pass_rows_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, words, n, cnt, rows);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
