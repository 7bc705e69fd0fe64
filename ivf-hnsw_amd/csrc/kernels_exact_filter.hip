// The base filter of the exact calls (ivfhnsw_gpu_set_base_filter) in its two forms in HBM.
//   pass words   one bit per row of the store, 32 to a word (word w = rows [32 w, 32 w + 32), the 32 columns of a sweep
//                tile), bits at or beyond n zero: the label bitmap launch_remove_bits makes (kernels_remove.hip), cut or
//                zero-extended to n rows, with the mode folded in -- deny inverts it.
//   pass rows    the passing row numbers ascending, from the words: a popcount per word, the exclusive scan of the
//                counts (launch_scan_excl_u32) and a scatter in which every row finds its place by the bits below it.
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

} // namespace

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
