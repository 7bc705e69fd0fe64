// Removing codes by label from the inverted lists a handle holds (ivfhnsw_gpu_remove_ids).  Every code
// whose id is one of the labels leaves its list; the others keep their order, so the new CSR is a stable compaction of
// the old one.  One unsharded handle only: its local rows are its global rows (loff[c] == goff[c]).
//   max      the largest label (the _dev form; the host form computes it on the host)
//   bits     a bitmap over [0, max label]: bit l set = label l is removed (global atomics)
//   mark     one workgroup per tile of kRemoveTileRows rows: every row's id against the bitmap, one ballot per 64 rows
//            into the removal mask (bit r = row r leaves), and keep[tile] = the rows of the tile that stay
//   counts   one wavefront per list: popcounts of the mask over the list's rows give rem[c]; on Grouping handles over
//            each sub-group's rows too, which gives the new sub-group sizes
//   scans    rem and keep become their exclusive scans (append's three-phase scan, kernels_append.hip)
//   offsets  goff'[c] = goff[c] - rem_scan[c], loff'[c] = loff[c] - rem_scan[c] (launch_update_offsets, kernels_append.hip)
//   compact  one workgroup per source tile: the ranks of its surviving rows from the mask, then the rows to the
//            contiguous range that starts at keep_scan[tile] (copy_gathered_rows, update_steps.h).  Destination dwords are
//            written in 16-byte aligned groups; a group the tile only partly owns gets dword stores (codes, ids) or byte
//            stores (norm codes) of its own part, so neighbouring tiles never write the same bytes.
// code_size is any multiple of 4, so a row is a whole number q of dwords: every address is dword aligned.
#include "ivfhnsw_kernels.h"
#include "update_steps.h"

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int kTileWords = kRemoveTileRows / 64; // mask words (64 rows each) per tile
static_assert(kTileWords <= 64 && kRemoveTileRows % 256 == 0, "one wavefront scans a tile's mask words");

__global__ __launch_bounds__(256) void remove_max_kernel(const uint32_t *__restrict__ labels, size_t n, uint32_t *__restrict__ out)
{
    uint32_t m = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
        m = max(m, labels[i]);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1)
        m = max(m, (uint32_t)__shfl_xor(m, o));
    if ((threadIdx.x & 63) == 0)
        atomicMax(out, m);
}

__global__ __launch_bounds__(256) void remove_bits_kernel(const uint32_t *__restrict__ labels, size_t n, uint32_t *__restrict__ bits)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t l = labels[i];
    atomicOr(bits + (l >> 5), 1u << (l & 31));
}

// wave w of the tile handles mask words w, w + 4, ...; each lane one row of a word
__global__ __launch_bounds__(256) void remove_mark_kernel(const uint32_t *__restrict__ ids, uint64_t n_local,
                                                          const uint32_t *__restrict__ bits, uint32_t max_label,
                                                          unsigned long long *__restrict__ mask, uint32_t *__restrict__ keep)
{
    __shared__ uint32_t s_keep[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int kIter = kTileWords / 4;
    const uint64_t w0 = (uint64_t)blockIdx.x * kTileWords;
    uint32_t id[kIter];
#pragma unroll
    for (int it = 0; it < kIter; it++) {
        const uint64_t r = (w0 + it * 4 + wave) * 64 + lane;
        id[it] = r < n_local ? ids[r] : 0u;
    }
    bool rm[kIter];
#pragma unroll
    for (int it = 0; it < kIter; it++) {
        const uint64_t r = (w0 + it * 4 + wave) * 64 + lane;
        rm[it] = r < n_local && id[it] <= max_label && ((bits[id[it] >> 5] >> (id[it] & 31)) & 1u);
    }
    uint32_t kept = 0;
#pragma unroll
    for (int it = 0; it < kIter; it++) {
        const uint64_t w = w0 + it * 4 + wave;
        const unsigned long long b_rm = __ballot(rm[it]);
        const unsigned long long b_in = __ballot(w * 64 + lane < n_local);
        if (lane == 0)
            mask[w] = b_rm;
        kept += (uint32_t)__popcll(b_in & ~b_rm);
    }
    if (lane == 0)
        s_keep[wave] = kept;
    __syncthreads();
    if (threadIdx.x == 0)
        keep[blockIdx.x] = s_keep[0] + s_keep[1] + s_keep[2] + s_keep[3];
}

// removed rows in [a, b), summed over the wavefront (every lane gets the total)
__device__ __forceinline__ uint32_t wave_removed(const unsigned long long *__restrict__ mask, uint64_t a, uint64_t b, int lane)
{
    uint32_t s = 0;
    if (a < b) {
        const uint64_t wa = a >> 6, wb = (b - 1) >> 6;
        for (uint64_t w = wa + lane; w <= wb; w += 64) {
            unsigned long long m = mask[w];
            if (w == wa)
                m &= ~0ull << (a & 63);
            if (w == wb)
                m &= ~0ull >> (63 - ((b - 1) & 63));
            s += (uint32_t)__popcll(m);
        }
    }
    return wave_sum(s);
}

// wave c: rem[c] (and rem_out[c]) = removed codes of list c; sizes != null: sizes2[c][j] = sizes[c][j] - removed codes of
// sub-group j.  Wave nc writes the scan's total slot rem[nc] = 0.
__global__ __launch_bounds__(256) void remove_counts_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ loff,
                                                            uint32_t nc, const unsigned long long *__restrict__ mask,
                                                            const uint32_t *__restrict__ sizes, uint32_t *__restrict__ sizes2,
                                                            int nsubc, uint32_t *__restrict__ rem, uint32_t *__restrict__ rem_out)
{
    const int lane = threadIdx.x & 63;
    const uint64_t c = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c > nc)
        return;
    if (c == nc) {
        if (lane == 0)
            rem[nc] = 0;
        return;
    }
    const uint64_t lo = loff[c], hi = lo + (goff[c + 1] - goff[c]);
    uint32_t tot = 0;
    if (sizes) {
        uint64_t a = lo;
        for (int j = 0; j < nsubc; j++) {
            const uint32_t sz = sizes[c * nsubc + j];
            const uint32_t r = sz ? wave_removed(mask, a, a + sz, lane) : 0u;
            if (lane == 0)
                sizes2[c * nsubc + j] = sz - r;
            a += sz;
            tot += r;
        }
    } else {
        tot = wave_removed(mask, lo, hi, lane);
    }
    if (lane == 0) {
        rem[c] = tot;
        if (rem_out)
            rem_out[c] = tot;
    }
}

// one workgroup per source tile; every lane of wavefront 0 takes part in the scan of the tile's mask words
__global__ __launch_bounds__(256) void remove_compact_kernel(const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ kscan,
                                                             uint64_t n_local, const uint32_t *__restrict__ codes,
                                                             const uint8_t *__restrict__ ncodes, const uint32_t *__restrict__ ids,
                                                             uint32_t *__restrict__ codes2, uint8_t *__restrict__ ncodes2,
                                                             uint32_t *__restrict__ ids2, uint32_t q)
{
    __shared__ uint32_t s_src[kRemoveTileRows];
    __shared__ unsigned long long s_keep[kTileWords];
    __shared__ uint32_t s_pre[kTileWords + 1];
    const uint64_t r0 = (uint64_t)blockIdx.x * kRemoveTileRows;
    if (threadIdx.x < 64) { // the tile's surviving rows per mask word, scanned across the wavefront
        const int lane = threadIdx.x;
        unsigned long long kb = 0;
        const uint64_t rw = r0 + (uint64_t)lane * 64;
        if (lane < kTileWords && rw < n_local) {
            kb = ~mask[(uint64_t)blockIdx.x * kTileWords + lane];
            if (n_local - rw < 64)
                kb &= (1ull << (n_local - rw)) - 1ull;
        }
        const uint32_t cnt = (uint32_t)__popcll(kb);
        const uint32_t inc = wave_incl_scan(cnt, lane);
        if (lane < kTileWords) {
            s_keep[lane] = kb;
            s_pre[lane] = inc - cnt;
        }
        if (lane == kTileWords - 1)
            s_pre[kTileWords] = inc;
    }
    __syncthreads();
    const uint32_t rows = s_pre[kTileWords];
    if (rows == 0)
        return;
    for (uint32_t j = threadIdx.x; j < (uint32_t)kRemoveTileRows; j += 256) {
        const uint32_t w = j >> 6, b = j & 63;
        const unsigned long long kb = s_keep[w];
        if ((kb >> b) & 1ull)
            s_src[kept_rank(s_pre[w], kb, b)] = (uint32_t)(r0 + j);
    }
    __syncthreads();
    copy_gathered_rows<false>(codes, ncodes, ids, codes2, ncodes2, ids2, s_src, rows, q, kscan[blockIdx.x]);
}

} // namespace

hipError_t launch_remove_max(hipStream_t s, const uint32_t *labels, size_t n, uint32_t *out)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(remove_max_kernel, dim3(blocks_of(n, 256) < 4096u ? blocks_of(n, 256) : 4096u), dim3(256), 0, s, labels,
                       n, out);
    return hipGetLastError();
}

hipError_t launch_remove_bits(hipStream_t s, const uint32_t *labels, size_t n, uint32_t max_label, uint32_t *bits)
{
    if (hipError_t e = hipMemsetAsync(bits, 0, ((size_t)max_label / 32 + 1) * sizeof(uint32_t), s); e != hipSuccess)
        return e;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(remove_bits_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, labels, n, bits);
    return hipGetLastError();
}

hipError_t launch_remove_mark(hipStream_t s, const IvfTables &t, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                              unsigned long long *mask, uint32_t *keep)
{
    if (n_local == 0)
        return hipSuccess;
    hipLaunchKernelGGL(remove_mark_kernel, dim3(blocks_of(n_local, kRemoveTileRows)), dim3(256), 0, s, t.ids, n_local, bits,
                       max_label, mask, keep);
    return hipGetLastError();
}

hipError_t launch_remove_counts(hipStream_t s, const IvfTables &t, const unsigned long long *mask, const uint32_t *sizes,
                                uint32_t *sizes2, int nsubc, uint32_t *rem, uint32_t *rem_out)
{
    hipLaunchKernelGGL(remove_counts_kernel, dim3(blocks_of((size_t)t.nc + 1, 4)), dim3(256), 0, s, t.goff, t.loff, t.nc, mask,
                       sizes, sizes2, nsubc, rem, rem_out);
    return hipGetLastError();
}

hipError_t launch_remove_compact(hipStream_t s, const IvfTables &t, uint64_t n_local, const unsigned long long *mask,
                                 const uint32_t *rscan, const uint32_t *kscan, const NewLists &nl)
{
    if (hipError_t e = launch_update_offsets(s, t, rscan, nullptr, false, nl); e != hipSuccess)
        return e;
    if (nl.n_local == 0)
        return hipSuccess;
    if (t.M % 4)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(remove_compact_kernel, dim3(blocks_of(n_local, kRemoveTileRows)), dim3(256), 0, s, mask, kscan, n_local,
                       reinterpret_cast<const uint32_t *>(t.codes), t.norm_codes, t.ids, reinterpret_cast<uint32_t *>(nl.codes),
                       nl.ncodes, nl.ids, (uint32_t)(t.M / 4));
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
