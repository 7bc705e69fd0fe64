// The row mask of a label filter (ivfhnsw_gpu_set_filter).  The labels go into a bitmap over
// [0, max label] with removal's kernels (launch_remove_max / launch_remove_bits, kernels_remove.hip); the mark pass here
// tests every local row's id against it and writes the PASS mask the filtered scans read: bit r = row r passes, one
// __ballot per 64 rows, bits at or beyond n_local zero.  Allow: a row passes iff its id is in the set; deny: iff it is
// not.  One workgroup per kFilterTileRows rows, one atomic per workgroup for the count of passing rows.
// Below them the kernels of the row tags: the scatter of (label, tag) pairs into the tag table with its
// conflict check, the gather of the table into one tag per resident row, and the counting pass.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int kFilterTileRows = 2048;
constexpr int kFilterTileWords = kFilterTileRows / 64;
constexpr int kFilterIter = kFilterTileWords / 4; // words per wavefront

// wave w of the tile handles mask words w, w + 4, ...; each lane one row of a word
__global__ __launch_bounds__(256) void filter_mark_kernel(const uint32_t *__restrict__ ids, uint64_t n_local, uint64_t nwords,
                                                          const uint32_t *__restrict__ bits, uint32_t max_label, int deny,
                                                          unsigned long long *__restrict__ mask,
                                                          unsigned long long *__restrict__ count)
{
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * kFilterTileWords;
    uint32_t id[kFilterIter];
#pragma unroll
    for (int it = 0; it < kFilterIter; it++) {
        const uint64_t r = (w0 + it * 4 + wave) * 64 + lane;
        id[it] = r < n_local ? ids[r] : 0u;
    }
    uint32_t passing = 0;
#pragma unroll
    for (int it = 0; it < kFilterIter; it++) {
        const uint64_t w = w0 + it * 4 + wave; // wave-uniform
        const uint64_t r = w * 64 + lane;
        const bool in_set = bits != nullptr && id[it] <= max_label && ((bits[id[it] >> 5] >> (id[it] & 31)) & 1u);
        const bool pass = r < n_local && (in_set != (deny != 0));
        const unsigned long long b = __ballot(pass);
        if (lane == 0 && w < nwords)
            mask[w] = b;
        passing += (uint32_t)__popcll(b);
    }
    if (lane == 0)
        s_cnt[wave] = passing;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t c = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (c)
            atomicAdd(count, (unsigned long long)c);
    }
}

// Every installed slot's plane in one pass: an update re-marks up to 32 label sets over the same ids, and
// a pass per slot would read the 4-byte ids once per slot.  The ids are read once, as above; each wavefront then ballots
// its 64 rows against one slot's bitmap after the other and writes one word per plane.  A plane below nplanes whose slot
// is not set is written zero, so the planes need no memset.  Passing counts: per wavefront in registers, per workgroup in
// LDS, one atomic per workgroup and installed slot.
__global__ __launch_bounds__(256) void filter_mark_slots_kernel(const uint32_t *__restrict__ ids, uint64_t n_local,
                                                                uint64_t nwords, FilterSlotSets sets, uint32_t nplanes,
                                                                unsigned long long *__restrict__ planes, uint64_t stride64,
                                                                unsigned long long *__restrict__ counts)
{
    __shared__ uint32_t s_cnt[kFilterSlots][4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t w0 = (uint64_t)blockIdx.x * kFilterTileWords;
    uint32_t id[kFilterIter];
#pragma unroll
    for (int it = 0; it < kFilterIter; it++) {
        const uint64_t r = (w0 + it * 4 + wave) * 64 + lane;
        id[it] = r < n_local ? ids[r] : 0u;
    }
    for (uint32_t s = 0; s < nplanes; s++) { // wave-uniform: the sets are kernel arguments
        const uint32_t *__restrict__ bits = sets.bits[s];
        const uint32_t max_label = sets.max_label[s];
        const bool set = sets.set[s] != 0, deny = sets.deny[s] != 0;
        unsigned long long *__restrict__ plane = planes + (size_t)s * stride64;
        uint32_t passing = 0;
#pragma unroll
        for (int it = 0; it < kFilterIter; it++) {
            const uint64_t w = w0 + it * 4 + wave;
            const uint64_t r = w * 64 + lane;
            const bool in_set = bits != nullptr && id[it] <= max_label && ((bits[id[it] >> 5] >> (id[it] & 31)) & 1u);
            const bool pass = set && r < n_local && (in_set != deny);
            const unsigned long long b = __ballot(pass);
            if (lane == 0 && w < nwords)
                plane[w] = b;
            passing += (uint32_t)__popcll(b);
        }
        if (lane == 0)
            s_cnt[s][wave] = passing;
    }
    __syncthreads();
    if (threadIdx.x < nplanes) {
        const uint32_t s = threadIdx.x;
        const uint32_t c = s_cnt[s][0] + s_cnt[s][1] + s_cnt[s][2] + s_cnt[s][3];
        if (c)
            atomicAdd(&counts[s], (unsigned long long)c);
    }
}

// ---- row tags: a uint16 per label value (the table), gathered into a uint16 per resident row

// table[labels[i]] = tags[i].  The table spans every label given (the host sized it by their maximum).  Two rows of the
// table share a 32-bit word; a 16-bit store touches its own half only, so threads that write neighbours do not meet.
__global__ __launch_bounds__(256) void tags_scatter_kernel(const uint32_t *__restrict__ labels, const uint16_t *__restrict__ tags,
                                                           size_t n, uint16_t *__restrict__ table)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        table[labels[i]] = tags[i];
}

// ... and the check behind it: a label given two different tags kept one of them, so the other entry does not read back
__global__ __launch_bounds__(256) void tags_verify_kernel(const uint32_t *__restrict__ labels, const uint16_t *__restrict__ tags,
                                                          size_t n, const uint16_t *__restrict__ table, uint32_t *__restrict__ conflict)
{
    const size_t stride = (size_t)gridDim.x * 256;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        bad |= table[labels[i]] != tags[i];
    if (bad)
        atomicOr(conflict, 1u);
}

// row_tags[r] = ids[r] < table_n ? table[ids[r]] : none.  A thread owns one 32-bit word of row_tags, rows 2w and 2w + 1;
// the last word of an odd n_local is stored as a half, the array ends there.
__global__ __launch_bounds__(256) void tags_gather_kernel(const uint32_t *__restrict__ ids, uint64_t n_local,
                                                          const uint16_t *__restrict__ table, uint64_t table_n,
                                                          uint16_t *__restrict__ row_tags)
{
    const uint64_t w = (uint64_t)blockIdx.x * 256 + threadIdx.x, r = 2 * w;
    if (r >= n_local)
        return;
    const bool two = r + 1 < n_local;
    const uint32_t i0 = ids[r], i1 = two ? ids[r + 1] : 0u;
    const uint32_t t0 = i0 < table_n ? table[i0] : 0xffffu;
    const uint32_t t1 = two && i1 < table_n ? table[i1] : 0xffffu;
    if (two)
        reinterpret_cast<uint32_t *>(row_tags)[w] = t0 | (t1 << 16);
    else
        row_tags[r] = (uint16_t)t0;
}

// *count += rows whose tag equals `tag` (equal) or differs from it (!equal): a ballot per wavefront, one atomic per workgroup
__global__ __launch_bounds__(256) void tags_count_kernel(const uint16_t *__restrict__ row_tags, uint64_t n_local, uint32_t tag,
                                                         int equal, unsigned long long *__restrict__ count)
{
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    uint32_t c = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < n_local; r0 += stride) { // workgroup-uniform bound: every lane ballots
        const uint64_t r = r0 + threadIdx.x;
        const bool hit = r < n_local && ((row_tags[r] == tag) == (equal != 0));
        c += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0)
        s_cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (t)
            atomicAdd(count, (unsigned long long)t);
    }
}

// ---- row values: a uint32 per label value (the table), gathered into a uint32 per resident row.  The
// tag kernels above are not generalised over the element type: the tag gather packs two rows into one 32-bit store and the
// tag count compares for equality, where a value row is a word of its own and is judged against an interval; the scatter
// and the verify differ in the element type alone, but as templates they would change the names the tag forms are compiled
// under, and the kernels that existed keep theirs.

// table[labels[i]] = values[i]; the table spans every label given
__global__ __launch_bounds__(256) void values_scatter_kernel(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ values,
                                                             size_t n, uint32_t *__restrict__ table)
{
    const size_t stride = (size_t)gridDim.x * 256;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        table[labels[i]] = values[i];
}

// ... and the check behind it: a label given two different values kept one of them, so the other entry does not read back
__global__ __launch_bounds__(256) void values_verify_kernel(const uint32_t *__restrict__ labels, const uint32_t *__restrict__ values,
                                                            size_t n, const uint32_t *__restrict__ table, uint32_t *__restrict__ conflict)
{
    const size_t stride = (size_t)gridDim.x * 256;
    bool bad = false;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += stride)
        bad |= table[labels[i]] != values[i];
    if (bad)
        atomicOr(conflict, 1u);
}

// row_values[r] = ids[r] < table_n ? table[ids[r]] : none
__global__ __launch_bounds__(256) void values_gather_kernel(const uint32_t *__restrict__ ids, uint64_t n_local,
                                                            const uint32_t *__restrict__ table, uint64_t table_n,
                                                            uint32_t *__restrict__ row_values)
{
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x; r < n_local; r += stride) {
        const uint32_t id = ids[r];
        row_values[r] = id < table_n ? table[id] : kValueNone;
    }
}

// *count += rows whose value lies in [lo, hi] (value_math.h): a ballot per wavefront, one atomic per workgroup
__global__ __launch_bounds__(256) void values_count_kernel(const uint32_t *__restrict__ row_values, uint64_t n_local, uint32_t lo,
                                                           uint32_t hi, unsigned long long *__restrict__ count)
{
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const ValueFill f = value_fill(lo, hi, true);
    uint32_t c = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < n_local; r0 += stride) { // workgroup-uniform bound: every lane ballots
        const uint64_t r = r0 + threadIdx.x;
        const bool hit = r < n_local && value_pass(row_values[r], f);
        c += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0)
        s_cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (t)
            atomicAdd(count, (unsigned long long)t);
    }
}

// *count += rows the conjunction of DESIGN.md 3.26 passes (tag_value_math.h), built as values_count_kernel is.  Either row
// array may be null: the lanes then read nothing of it and every row counts as untagged / without a value.
__global__ __launch_bounds__(256) void tag_values_count_kernel(const uint16_t *__restrict__ row_tags,
                                                               const uint32_t *__restrict__ row_values, uint64_t n_local,
                                                               uint32_t tag, uint32_t lo, uint32_t hi,
                                                               unsigned long long *__restrict__ count)
{
    __shared__ uint32_t s_cnt[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    const TagValueFill f = tag_value_fill(tag, lo, hi, row_tags != nullptr, row_values != nullptr);
    uint32_t c = 0;
    for (uint64_t r0 = (uint64_t)blockIdx.x * 256; r0 < n_local; r0 += stride) { // workgroup-uniform bound: every lane ballots
        const uint64_t r = r0 + threadIdx.x;
        bool hit = false;
        if (r < n_local) {
            const uint32_t wt = row_tags ? (uint32_t)row_tags[r] : 0u; // without the array the word is ignored: f.tag has bit 16 set or is the wildcard
            const uint32_t wv = row_values ? row_values[r] : 0u;       // ... and f.value.keep = 0 makes it 0xffffffff
            hit = tag_value_pass(wt, wv, f);
        }
        c += (uint32_t)__popcll(__ballot(hit));
    }
    if (lane == 0)
        s_cnt[wave] = c;
    __syncthreads();
    if (threadIdx.x == 0) {
        const uint32_t t = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
        if (t)
            atomicAdd(count, (unsigned long long)t);
    }
}

} // namespace

static unsigned tags_grid(uint64_t n) { return (unsigned)std::min<uint64_t>((n + 255) / 256, 1u << 16); }

hipError_t launch_tags_scatter(hipStream_t s, const uint32_t *labels, const uint16_t *tags, size_t n, uint16_t *table,
                               uint32_t *conflict)
{
    if (hipError_t e = hipMemsetAsync(conflict, 0, sizeof(uint32_t), s); e != hipSuccess)
        return e;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(tags_scatter_kernel, dim3(tags_grid(n)), dim3(256), 0, s, labels, tags, n, table);
    hipLaunchKernelGGL(tags_verify_kernel, dim3(tags_grid(n)), dim3(256), 0, s, labels, tags, n, table, conflict);
    return hipGetLastError();
}

hipError_t launch_tags_gather(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint16_t *table, uint64_t table_n,
                              uint16_t *row_tags)
{
    if (n_local == 0) // the one element the array always has
        return hipMemsetAsync(row_tags, 0xff, sizeof(uint16_t), s);
    const uint64_t words = (n_local + 1) / 2;
    hipLaunchKernelGGL(tags_gather_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, ids, n_local, table, table_n,
                       row_tags);
    return hipGetLastError();
}

hipError_t launch_tags_count(hipStream_t s, const uint16_t *row_tags, uint64_t n_local, uint32_t tag, bool equal,
                             unsigned long long *count)
{
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), s); e != hipSuccess)
        return e;
    if (n_local == 0)
        return hipSuccess;
    hipLaunchKernelGGL(tags_count_kernel, dim3(tags_grid(n_local)), dim3(256), 0, s, row_tags, n_local, tag, equal ? 1 : 0, count);
    return hipGetLastError();
}

hipError_t launch_values_scatter(hipStream_t s, const uint32_t *labels, const uint32_t *values, size_t n, uint32_t *table,
                                 uint32_t *conflict)
{
    if (hipError_t e = hipMemsetAsync(conflict, 0, sizeof(uint32_t), s); e != hipSuccess)
        return e;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(values_scatter_kernel, dim3(tags_grid(n)), dim3(256), 0, s, labels, values, n, table);
    hipLaunchKernelGGL(values_verify_kernel, dim3(tags_grid(n)), dim3(256), 0, s, labels, values, n, table, conflict);
    return hipGetLastError();
}

hipError_t launch_values_gather(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint32_t *table, uint64_t table_n,
                                uint32_t *row_values)
{
    if (n_local == 0) // the one element the array always has
        return hipMemsetAsync(row_values, 0xff, sizeof(uint32_t), s);
    hipLaunchKernelGGL(values_gather_kernel, dim3(tags_grid(n_local)), dim3(256), 0, s, ids, n_local, table, table_n, row_values);
    return hipGetLastError();
}

hipError_t launch_values_count(hipStream_t s, const uint32_t *row_values, uint64_t n_local, uint32_t lo, uint32_t hi,
                               unsigned long long *count)
{
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), s); e != hipSuccess)
        return e;
    if (n_local == 0)
        return hipSuccess;
    hipLaunchKernelGGL(values_count_kernel, dim3(tags_grid(n_local)), dim3(256), 0, s, row_values, n_local, lo, hi, count);
    return hipGetLastError();
}

hipError_t launch_tag_values_count(hipStream_t s, const uint16_t *row_tags, const uint32_t *row_values, uint64_t n_local,
                                   uint32_t tag, uint32_t lo, uint32_t hi, unsigned long long *count)
{
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), s); e != hipSuccess)
        return e;
    if (n_local == 0)
        return hipSuccess;
    hipLaunchKernelGGL(tag_values_count_kernel, dim3(tags_grid(n_local)), dim3(256), 0, s, row_tags, row_values, n_local, tag, lo,
                       hi, count);
    return hipGetLastError();
}

hipError_t launch_filter_mark(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                              int deny, unsigned long long *mask, unsigned long long *count)
{
    if (hipError_t e = hipMemsetAsync(count, 0, sizeof(unsigned long long), s); e != hipSuccess)
        return e;
    if (n_local == 0)
        return hipSuccess;
    const uint64_t nwords = (n_local + 63) / 64;
    const unsigned grid = (unsigned)((n_local + kFilterTileRows - 1) / kFilterTileRows);
    hipLaunchKernelGGL(filter_mark_kernel, dim3(grid), dim3(256), 0, s, ids, n_local, nwords, bits, max_label, deny, mask, count);
    return hipGetLastError();
}

hipError_t launch_filter_mark_slots(hipStream_t s, const uint32_t *ids, uint64_t n_local, const FilterSlotSets &sets,
                                    uint32_t nplanes, unsigned long long *planes, uint64_t stride64,
                                    unsigned long long *counts)
{
    if (nplanes > (uint32_t)kFilterSlots)
        return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(counts, 0, kFilterSlots * sizeof(unsigned long long), s); e != hipSuccess)
        return e;
    const uint64_t nwords = (n_local + 63) / 64;
    if (n_local == 0 || nplanes == 0)
        return hipSuccess;
    if (nwords > stride64)
        return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n_local + kFilterTileRows - 1) / kFilterTileRows);
    hipLaunchKernelGGL(filter_mark_slots_kernel, dim3(grid), dim3(256), 0, s, ids, n_local, nwords, sets, nplanes, planes,
                       stride64, counts);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
