// The base filter of the exact calls (ivfhnsw_gpu_set_base_filter) in its two forms in HBM.
//   pass words   one bit per row of the store, 32 to a word (word w = rows [32 w, 32 w + 32), the 32 columns of a sweep
//                tile), bits at or beyond n zero: the label bitmap launch_remove_bits makes (kernels_remove.hip), cut or
//                zero-extended to n rows, with the mode folded in -- deny inverts it.
//   pass rows    the passing row numbers ascending, from the words: a popcount per word, the exclusive scan of the
//                counts (launch_scan_excl_u32) and a scatter in which every row finds its place by the bits below it.
// Below them the strip plan of a call with a base filter slot per query: count, layout, scatter.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

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

} // namespace

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
