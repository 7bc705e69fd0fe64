// Replacing codes by label in the inverted lists a handle holds (ivfhnsw_gpu_upsert_ivf): every code whose
// id is one of the batch's labels leaves its list, and batch code i goes to the end of list list_idx[i].  The result is
// that of a removal (kernels_remove.hip) followed by an append (kernels_append.hip), built in ONE pass: every old row is
// read once, every new row written once, and no intermediate lists exist.  One unsharded IVFADC handle only.
//   bits     the label bitmap as removal builds it; an atomic OR that finds its bit set saw a label twice: *status
//   mark, counts, scans, sort, count
//            removal's and append's own steps: mask, keep -> kscan, rem -> rscan, cnt -> nstart, perm
//   offsets  goff'[c] = goff[c] - rscan[c] + nstart[c], loff' the same (upsert_list_start, update_math.h)
//   tiles    tile_first[t] = the old list that holds row t * kRemoveTileRows
//   compact  one workgroup per SOURCE tile: the ranks of its surviving rows from the mask, as the removal's compaction;
//            then the tile is split at the list boundaries inside it (tile_segment), and the kept rows of each (tile, list)
//            segment go to the contiguous range that starts at kscan[tile] + rank + nstart[list] (copy_gathered_rows).
//            Between two segments lie the places of the batch's rows, which this kernel does not touch
//   scatter  row p of the sorted batch goes behind the kept rows of its list (upsert_batch_dest): dword stores for codes
//            and ids, byte stores for norm codes
// A segment's range is written in 16-byte groups where it owns the group and in dwords (codes, ids) or bytes (norm codes)
// at its ends, so no two workgroups and no two kernels write the same byte, and nothing is read, modified and written.
// code_size is any multiple of 4: every address is dword aligned.
#include "ivfhnsw_kernels.h"
#include "update_steps.h"

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int kTileWords = kRemoveTileRows / 64; // mask words (64 rows each) per tile
static_assert(kTileWords <= 64 && kRemoveTileRows % 256 == 0, "one wavefront scans a tile's mask words");

__global__ __launch_bounds__(256) void upsert_bits_kernel(const uint32_t *__restrict__ labels, size_t n, uint32_t *__restrict__ bits,
                                                          uint32_t *__restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t l = labels[i], b = 1u << (l & 31);
    if (atomicOr(bits + (l >> 5), b) & b)
        *status = 1u;
}

__global__ __launch_bounds__(256) void upsert_offsets_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ loff,
                                                             const uint32_t *__restrict__ rscan, const uint32_t *__restrict__ nstart,
                                                             uint64_t *__restrict__ goff2, uint32_t *__restrict__ loff2, uint32_t nc)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c > nc)
        return;
    goff2[c] = goff[c] - rscan[c] + nstart[c];
    if (c < nc)
        loff2[c] = upsert_list_start(loff[c], rscan[c], nstart[c]);
}

// tile_first[t] = the list holding old row t * kRemoveTileRows; tile_first[ntiles] = nc - 1
__global__ __launch_bounds__(256) void upsert_tiles_kernel(const uint32_t *__restrict__ loff, uint32_t nc, uint32_t ntiles,
                                                           uint32_t *__restrict__ tile_first)
{
    const uint32_t t = blockIdx.x * 256 + threadIdx.x;
    if (t > ntiles)
        return;
    tile_first[t] = t == ntiles ? nc - 1 : list_of_row(loff, 0u, nc - 1, t * (uint32_t)kRemoveTileRows);
}

// One workgroup per source tile; every lane of wavefront 0 takes part in the scan of the tile's mask words.  The segment
// loop's conditions are the same in every thread, and no barrier stands inside it.
__global__ __launch_bounds__(256) void upsert_compact_kernel(const unsigned long long *__restrict__ mask, const uint32_t *__restrict__ kscan,
                                                             const uint32_t *__restrict__ tile_first, const uint64_t *__restrict__ goff,
                                                             const uint32_t *__restrict__ loff, const uint32_t *__restrict__ nstart,
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
    if (s_pre[kTileWords] == 0)
        return;
    for (uint32_t j = threadIdx.x; j < (uint32_t)kRemoveTileRows; j += 256) {
        const uint32_t w = j >> 6, b = j & 63;
        const unsigned long long kb = s_keep[w];
        if ((kb >> b) & 1ull)
            s_src[kept_rank(s_pre[w], kb, b)] = (uint32_t)(r0 + j);
    }
    __syncthreads();
    const uint32_t a0 = (uint32_t)r0, r_end = (uint32_t)min(r0 + kRemoveTileRows, n_local);
    const uint32_t hi = tile_first[blockIdx.x + 1], base = kscan[blockIdx.x];
    uint32_t lo = tile_first[blockIdx.x], a = a0;
    while (a < r_end) {
        const TileSegment seg = tile_segment(loff, goff, lo, hi, a, r_end);
        if (seg.end <= a) // (tables that are no CSR: never with the handle's own)
            break;
        const uint32_t j0 = kept_before(s_pre, s_keep, a - a0, 6u, (uint32_t)kTileWords);
        const uint32_t j1 = kept_before(s_pre, s_keep, seg.end - a0, 6u, (uint32_t)kTileWords);
        if (j1 > j0)
            copy_gathered_rows<false>(codes, ncodes, ids, codes2, ncodes2, ids2, s_src + j0, j1 - j0, q,
                                      upsert_kept_dest(base, j0, nstart[seg.list]));
        lo = seg.list;
        a = seg.end;
    }
}

// one thread per dword of the new codes, in sorted order: code p of the sorted batch is input row perm[p]
__global__ __launch_bounds__(256) void upsert_scatter_kernel(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ list_idx,
                                                             const uint32_t *__restrict__ nstart, const uint32_t *__restrict__ rscan,
                                                             const uint32_t *__restrict__ loff, const uint64_t *__restrict__ goff,
                                                             const uint32_t *__restrict__ new_codes, const uint8_t *__restrict__ new_norm,
                                                             const uint32_t *__restrict__ new_ids, uint32_t *__restrict__ codes2,
                                                             uint8_t *__restrict__ ncodes2, uint32_t *__restrict__ ids2, size_t n, uint32_t q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * q)
        return;
    const size_t p = e / q;
    const uint32_t k = (uint32_t)(e - p * q);
    const uint32_t i = perm[p];
    const uint32_t c = list_idx[i];
    const size_t row = upsert_batch_dest(loff[c], (uint32_t)(goff[c + 1] - goff[c]), rscan[c], rscan[c + 1], p, nstart[c]);
    codes2[row * q + k] = new_codes[(size_t)i * q + k];
    if (k == 0) {
        ids2[row] = new_ids[i];
        ncodes2[row] = new_norm[i];
    }
}

} // namespace

hipError_t launch_upsert_bits(hipStream_t s, const uint32_t *labels, size_t n, uint32_t max_label, uint32_t *bits, uint32_t *status)
{
    if (hipError_t e = hipMemsetAsync(bits, 0, ((size_t)max_label / 32 + 1) * sizeof(uint32_t), s); e != hipSuccess)
        return e;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(upsert_bits_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, labels, n, bits, status);
    return hipGetLastError();
}

hipError_t launch_upsert_layout(hipStream_t s, const IvfTables &t, uint64_t n_local, const uint32_t *rscan, const uint32_t *nstart,
                                uint32_t *tile_first, const NewLists &nl)
{
    if (n_local >= 0xffffffffull || nl.n_local >= 0xffffffffull || t.M % 4)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsert_offsets_kernel, dim3(blocks_of((size_t)t.nc + 1, 256)), dim3(256), 0, s, t.goff, t.loff, rscan, nstart,
                       nl.goff, nl.loff, t.nc);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    const uint32_t ntiles = (uint32_t)blocks_of(n_local, kRemoveTileRows);
    hipLaunchKernelGGL(upsert_tiles_kernel, dim3(blocks_of((size_t)ntiles + 1, 256)), dim3(256), 0, s, t.loff, t.nc, ntiles, tile_first);
    return hipGetLastError();
}

hipError_t launch_upsert_compact(hipStream_t s, const IvfTables &t, uint64_t n_local, const unsigned long long *mask,
                                 const uint32_t *kscan, const uint32_t *nstart, const uint32_t *tile_first, const NewLists &nl)
{
    if (n_local == 0)
        return hipSuccess;
    if (n_local >= 0xffffffffull || t.M % 4)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(upsert_compact_kernel, dim3(blocks_of(n_local, kRemoveTileRows)), dim3(256), 0, s, mask, kscan, tile_first,
                       t.goff, t.loff, nstart, n_local, reinterpret_cast<const uint32_t *>(t.codes), t.norm_codes, t.ids,
                       reinterpret_cast<uint32_t *>(nl.codes), nl.ncodes, nl.ids, (uint32_t)(t.M / 4));
    return hipGetLastError();
}

hipError_t launch_upsert_scatter(hipStream_t s, const IvfTables &t, const uint32_t *perm, const uint32_t *list_idx, size_t n,
                                 const uint32_t *nstart, const uint32_t *rscan, const uint8_t *codes, const uint8_t *norm_codes,
                                 const uint32_t *ids, const NewLists &nl)
{
    if (n == 0)
        return hipSuccess;
    const uint32_t q = (uint32_t)(t.M / 4);
    hipLaunchKernelGGL(upsert_scatter_kernel, dim3(blocks_of(n * q, 256)), dim3(256), 0, s, perm, list_idx, nstart, rscan, t.loff,
                       t.goff, reinterpret_cast<const uint32_t *>(codes), norm_codes, ids, reinterpret_cast<uint32_t *>(nl.codes), nl.ncodes,
                       nl.ids, n, q);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
