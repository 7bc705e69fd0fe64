// The row mask of a label filter (ivfhnsw_gpu_set_filter).  The labels go into a bitmap over
// [0, max label] with removal's kernels (launch_remove_max / launch_remove_bits, kernels_remove.hip); the mark pass here
// tests every local row's id against it and writes the PASS mask the filtered scans read: bit r = row r passes, one
// __ballot per 64 rows, bits at or beyond n_local zero.  Allow: a row passes iff its id is in the set; deny: iff it is
// not.  One workgroup per kFilterTileRows rows, one atomic per workgroup for the count of passing rows.
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

} // namespace

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
