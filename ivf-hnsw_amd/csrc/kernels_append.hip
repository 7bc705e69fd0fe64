// Appending codes to the inverted lists a handle holds (ivfhnsw_gpu_append_ivf).  The reference's
// add_batch appends code i to the end of list idx[i], in input order (IndexIVF_HNSW.cpp:122-131); the lists only grow
// at their ends, so the new CSR is the old one with every list stretched.  One out-of-place merge builds it:
//   count    cnt[c] = new codes of list c (global atomics); an id >= nc raises *status and is not counted
//   lens     own[c] = old length + cnt[c] for the lists this shard owns (loff[c] != kNotOwned), 0 otherwise
//   scan     nstart = exclusive scan of cnt, lstart = exclusive scan of own (both [nc + 1]; lstart[nc] = the new n_local)
//   offsets  goff'[c] = goff[c] + nstart[c]; loff'[c] = lstart[c] for owned lists, kNotOwned for the others
//   merge    old row r of list c moves to r + (lstart[c] - loff[c]): a destination-tiled copy.  Each workgroup reads the
//            first list of its tile (tile_first, one binary search per tile) and finds every row's list within the
//            tile's range; the rows are then copied as 16-byte groups (codes, ids) and 4-byte groups (norm codes).
//            The tile's new rows get zeros; the scatter below overwrites them
//   scatter  new code p of the stably sorted batch (launch_sort_by_key, kernels_kmeans.hip) goes to
//            lstart[c] + old_len[c] + (p - nstart[c])
// A Grouping list is nsubc sub-groups laid end to end and grows at the end of each of them (DESIGN.md 3.12,
// kernels_add_groups.hip): count, merge and scatter take the sub-group tables as SubGroups and are the same kernels.
// code_size is any multiple of 4, so a row is a whole number q of dwords but not always of 16-byte groups: every
// address here is dword aligned, and the merge's destination groups are 16-byte aligned (a tile is 2048 rows).
#include "ivfhnsw_kernels.h"
#include "update_steps.h"

namespace ivfhnsw_gpu_impl {

namespace {

// cnt[list] += 1 per batch row, and with sub_idx sizes2[list][sub] += 1; cnt null: the id check alone
__global__ __launch_bounds__(256) void append_count_kernel(const uint32_t *__restrict__ list_idx, const uint32_t *__restrict__ sub_idx,
                                                           size_t n, uint32_t nc, uint32_t nsubc, uint32_t *__restrict__ cnt,
                                                           uint32_t *__restrict__ sizes2, uint32_t *__restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t c = list_idx[i], s = sub_idx ? sub_idx[i] : 0u;
    if (c >= nc || (sub_idx && s >= nsubc)) {
        *status = 1u;
    } else if (cnt) {
        atomicAdd(cnt + c, 1u);
        if (sizes2)
            atomicAdd(sizes2 + (size_t)c * nsubc + s, 1u);
    }
}

// own[c] for c < nc (own[nc] = 0, the scan's total slot)
__global__ __launch_bounds__(256) void append_lens_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ loff,
                                                          const uint32_t *__restrict__ cnt, uint32_t *__restrict__ own,
                                                          uint32_t nc)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c > nc)
        return;
    own[c] = (c < nc && loff[c] != kNotOwned) ? (uint32_t)(goff[c + 1] - goff[c]) + cnt[c] : 0u;
}

// exclusive scan of [len] in chunks of kScanChunk: part[b] = sum of chunk b, then (part scanned) each chunk in place.
// blockIdx.y picks the array (a or b), so both scans share the launches.  Every thread of both kernels reaches
// block_excl_scan (elements past len count 0).
__global__ __launch_bounds__(256) void scan_reduce_kernel(const uint32_t *__restrict__ a, const uint32_t *__restrict__ b,
                                                          size_t len, uint32_t *__restrict__ part, uint32_t nblk)
{
    __shared__ uint32_t s_w[4];
    const uint32_t *x = blockIdx.y ? b : a;
    const size_t i0 = (size_t)blockIdx.x * kScanChunk;
    uint32_t acc = 0;
    for (int r = 0; r < kScanChunk / 256; r++) {
        const size_t i = i0 + (size_t)r * 256 + threadIdx.x;
        if (i < len)
            acc += x[i];
    }
    uint32_t total;
    (void)block_excl_scan<4>(acc, s_w, total);
    if (threadIdx.x == 0)
        part[(size_t)blockIdx.y * nblk + blockIdx.x] = total;
}

// each thread owns 16 consecutive elements of the chunk
__global__ __launch_bounds__(256) void scan_apply_kernel(uint32_t *__restrict__ a, uint32_t *__restrict__ b, size_t len,
                                                         const uint32_t *__restrict__ part, uint32_t nblk)
{
    __shared__ uint32_t s_w[4];
    uint32_t *x = blockIdx.y ? b : a;
    const size_t i0 = (size_t)blockIdx.x * kScanChunk + (size_t)threadIdx.x * 16;
    uint32_t v[16], s = 0;
#pragma unroll
    for (int u = 0; u < 16; u++) {
        v[u] = i0 + u < len ? x[i0 + u] : 0u;
        s += v[u];
    }
    uint32_t total;
    uint32_t run = part[(size_t)blockIdx.y * nblk + blockIdx.x] + block_excl_scan<4>(s, s_w, total);
#pragma unroll
    for (int u = 0; u < 16; u++) {
        if (i0 + u < len)
            x[i0 + u] = run;
        run += v[u];
    }
}

// The new offsets of every list from the exclusive scan `delta` of what each list gains (grow: the batch's rows per list)
// or loses (the removed rows per list).  lstart (an append: the new local starts, which count owned lists only) null:
// the local start moves by delta as the global one does (a removal, whose handle owns every list).
__global__ __launch_bounds__(256) void update_offsets_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ loff,
                                                             const uint32_t *__restrict__ delta, const uint32_t *__restrict__ lstart,
                                                             bool grow, uint64_t *__restrict__ goff2, uint32_t *__restrict__ loff2,
                                                             uint32_t nc)
{
    const size_t c = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (c > nc)
        return;
    goff2[c] = grow ? goff[c] + delta[c] : goff[c] - delta[c];
    if (c < nc)
        loff2[c] = loff[c] == kNotOwned ? kNotOwned : lstart ? lstart[c] : loff[c] - delta[c];
}

// tile_first[b] = the list holding row b * kAppendTileRows of the new local arrays; tile_first[ntiles] = nc - 1
__global__ __launch_bounds__(256) void append_tiles_kernel(const uint32_t *__restrict__ lstart, uint32_t nc, uint32_t ntiles,
                                                           uint32_t *__restrict__ tile_first)
{
    const uint32_t b = blockIdx.x * 256 + threadIdx.x;
    if (b > ntiles)
        return;
    tile_first[b] = b == ntiles ? nc - 1 : list_of_row(lstart, 0, nc - 1, b * (uint32_t)kAppendTileRows);
}

// One workgroup per tile of the new arrays: the source row of every tile row, then the copy.  GROUPING: a row of a list
// the batch touches (nstart[c + 1] > nstart[c]) finds its sub-group by one binary search over the list's nsubc new prefix
// sums; a row of an untouched list takes the IVFADC path (the list moves as a whole).  A tile whose lists' prefix sums
// fit kPrefixCache (the rule at the metric's shape: two to four lists of ~1000 rows per tile) loads them into LDS with
// coalesced, independent loads first, so that a row's search runs at LDS latency; a tile over many short lists searches
// in global memory.  The IVFADC kernel has neither the cache nor the branch.
template <bool GROUPING>
__global__ __launch_bounds__(256) void append_merge_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ loff,
                                                           const uint32_t *__restrict__ nstart, const uint32_t *__restrict__ lstart,
                                                           const uint32_t *__restrict__ tile_first, const SubGroups sg,
                                                           const uint32_t *__restrict__ codes, const uint8_t *__restrict__ ncodes,
                                                           const uint32_t *__restrict__ ids, uint32_t *__restrict__ codes2,
                                                           uint8_t *__restrict__ ncodes2, uint32_t *__restrict__ ids2,
                                                           uint32_t n_local2, uint32_t q)
{
    __shared__ uint32_t s_src[kAppendTileRows];
    const uint32_t r0 = blockIdx.x * (uint32_t)kAppendTileRows;
    const uint32_t rows = min((uint32_t)kAppendTileRows, n_local2 - r0);
    const uint32_t lo = tile_first[blockIdx.x], hi = tile_first[blockIdx.x + 1];
    const uint32_t nsubc = sg.nsubc;
    const uint32_t *s_pn = nullptr, *s_po = nullptr;
    uint32_t cached_words = 0;
    if constexpr (GROUPING) {
        __shared__ uint32_t s_pre[2][kPrefixCache];
        cached_words = prefix_cache_words(lo, hi, nsubc);
        for (uint32_t w = threadIdx.x; w < cached_words; w += 256) {
            const uint32_t c = lo + w / nsubc;
            if (nstart[c + 1] != nstart[c]) { // (untouched lists have no prefix rows)
                const size_t g = (size_t)c * nsubc + w % nsubc;
                s_pre[0][w] = sg.pre_new[g];
                s_pre[1][w] = sg.pre_old[g];
            }
        }
        __syncthreads();
        s_pn = s_pre[0];
        s_po = s_pre[1];
    }
    for (uint32_t j = threadIdx.x; j < rows; j += 256) {
        const uint32_t r = r0 + j;
        const uint32_t c = list_of_row(lstart, lo, hi, r);
        const uint32_t off = r - lstart[c];
        const uint32_t old_len = (uint32_t)(goff[c + 1] - goff[c]);
        uint32_t src;
        if (!GROUPING || nstart[c + 1] == nstart[c])
            src = list_source(off, old_len, loff[c]);
        else if (cached_words)
            src = grouping_source(s_pn + (c - lo) * nsubc, s_po + (c - lo) * nsubc, nsubc, off, old_len, loff[c]);
        else
            src = grouping_source(sg.pre_new + (size_t)c * nsubc, sg.pre_old + (size_t)c * nsubc, nsubc, off, old_len, loff[c]);
        s_src[j] = src;
    }
    __syncthreads();
    copy_gathered_rows<true>(codes, ncodes, ids, codes2, ncodes2, ids2, s_src, rows, q, r0);
}

// one thread per dword of the new codes, in sorted order: code p of the sorted batch is input row perm[p]
template <bool GROUPING>
__global__ __launch_bounds__(256) void append_scatter_kernel(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ list_idx,
                                                             const uint32_t *__restrict__ nstart, const uint32_t *__restrict__ loff,
                                                             const uint64_t *__restrict__ goff, const uint32_t *__restrict__ lstart,
                                                             const SubGroups sg, const uint32_t *__restrict__ new_codes,
                                                             const uint8_t *__restrict__ new_norm, const uint32_t *__restrict__ new_ids,
                                                             uint32_t *__restrict__ codes2, uint8_t *__restrict__ ncodes2,
                                                             uint32_t *__restrict__ ids2, size_t n, uint32_t q)
{
    const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (e >= n * q)
        return;
    const size_t p = e / q;
    const uint32_t k = (uint32_t)(e - p * q);
    const uint32_t i = perm[p];
    const uint32_t c = list_idx[i];
    if (loff[c] == kNotOwned)
        return;
    size_t row;
    if constexpr (GROUPING) {
        const size_t cs = (size_t)c * sg.nsubc + sg.sub_idx[i];
        row = grouping_dest_row(lstart[c], sg.pre_old[cs], sg.sizes[cs], p, nstart[c]);
    } else {
        row = append_dest_row(lstart[c], (uint32_t)(goff[c + 1] - goff[c]), p, nstart[c]);
    }
    codes2[row * q + k] = new_codes[(size_t)i * q + k];
    if (k == 0) {
        ids2[row] = new_ids[i];
        ncodes2[row] = new_norm[i];
    }
}

} // namespace

hipError_t launch_append_count(hipStream_t s, const uint32_t *list_idx, const uint32_t *sub_idx, size_t n, uint32_t nc,
                               uint32_t nsubc, uint32_t *cnt, uint32_t *sizes2, uint32_t *status)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(append_count_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, list_idx, sub_idx, n, nc, nsubc, cnt, sizes2,
                       status);
    return hipGetLastError();
}

// the three-phase exclusive scan of a (and of b beside it when non-null), [len] each, in place
static hipError_t scan_excl(hipStream_t s, uint32_t *a, uint32_t *b, size_t len, uint32_t *part)
{
    const uint32_t nblk = (uint32_t)blocks_of(len, kScanChunk), narr = b ? 2 : 1;
    hipLaunchKernelGGL(scan_reduce_kernel, dim3(nblk, narr), dim3(256), 0, s, a, b, len, part, nblk);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    for (uint32_t y = 0; y < narr; y++)
        if (hipError_t e = launch_scan_u32(s, part + y * nblk, part + y * nblk, nblk); e != hipSuccess)
            return e;
    hipLaunchKernelGGL(scan_apply_kernel, dim3(nblk, narr), dim3(256), 0, s, a, b, len, part, nblk);
    return hipGetLastError();
}

hipError_t launch_append_tables(hipStream_t s, const IvfTables &t, uint32_t *cnt, uint32_t *own, uint32_t *part)
{
    const size_t len = (size_t)t.nc + 1;
    hipLaunchKernelGGL(append_lens_kernel, dim3(blocks_of(len, 256)), dim3(256), 0, s, t.goff, t.loff, cnt, own, t.nc);
    if (hipError_t e = hipGetLastError(); e != hipSuccess)
        return e;
    return scan_excl(s, cnt, own, len, part);
}

hipError_t launch_scan_excl_u32(hipStream_t s, uint32_t *a, size_t len, uint32_t *part)
{
    return len ? scan_excl(s, a, nullptr, len, part) : hipSuccess;
}

hipError_t launch_update_offsets(hipStream_t s, const IvfTables &t, const uint32_t *delta, const uint32_t *lstart, bool grow,
                                 const NewLists &nl)
{
    hipLaunchKernelGGL(update_offsets_kernel, dim3(blocks_of((size_t)t.nc + 1, 256)), dim3(256), 0, s, t.goff, t.loff, delta,
                       lstart, grow, nl.goff, nl.loff, t.nc);
    return hipGetLastError();
}

hipError_t launch_append_layout(hipStream_t s, const IvfTables &t, const uint32_t *nstart, const uint32_t *lstart,
                                uint32_t *tile_first, const NewLists &nl)
{
    if (hipError_t e = launch_update_offsets(s, t, nstart, lstart, true, nl); e != hipSuccess)
        return e;
    if (nl.n_local == 0)
        return hipSuccess;
    if (nl.n_local >= 0xffffffffull || t.M % 4)
        return hipErrorInvalidValue;
    const uint32_t ntiles = (uint32_t)blocks_of(nl.n_local, kAppendTileRows);
    hipLaunchKernelGGL(append_tiles_kernel, dim3(blocks_of((size_t)ntiles + 1, 256)), dim3(256), 0, s, lstart, t.nc, ntiles,
                       tile_first);
    return hipGetLastError();
}

hipError_t launch_append_merge(hipStream_t s, const IvfTables &t, const uint32_t *nstart, const uint32_t *lstart,
                               const uint32_t *tile_first, const SubGroups *sg, const NewLists &nl)
{
    if (nl.n_local == 0)
        return hipSuccess;
    if (nl.n_local >= 0xffffffffull || t.M % 4 || (sg && sg->nsubc == 0))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sg ? append_merge_kernel<true> : append_merge_kernel<false>, dim3(blocks_of(nl.n_local, kAppendTileRows)),
                       dim3(256), 0, s, t.goff, t.loff, nstart, lstart, tile_first, sg ? *sg : SubGroups{},
                       reinterpret_cast<const uint32_t *>(t.codes), t.norm_codes, t.ids, reinterpret_cast<uint32_t *>(nl.codes),
                       nl.ncodes, nl.ids, (uint32_t)nl.n_local, (uint32_t)(t.M / 4));
    return hipGetLastError();
}

hipError_t launch_append_scatter(hipStream_t s, const IvfTables &t, const uint32_t *perm, const uint32_t *list_idx, size_t n,
                                 const uint32_t *nstart, const uint32_t *lstart, const SubGroups *sg, const uint8_t *codes,
                                 const uint8_t *norm_codes, const uint32_t *ids, const NewLists &nl)
{
    if (n == 0)
        return hipSuccess;
    const uint32_t q = (uint32_t)(t.M / 4);
    hipLaunchKernelGGL(sg ? append_scatter_kernel<true> : append_scatter_kernel<false>, dim3(blocks_of(n * q, 256)), dim3(256), 0,
                       s, perm, list_idx, nstart, t.loff, t.goff, lstart, sg ? *sg : SubGroups{},
                       reinterpret_cast<const uint32_t *>(codes), norm_codes, ids, reinterpret_cast<uint32_t *>(nl.codes),
                       nl.ncodes, nl.ids, n, q);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
