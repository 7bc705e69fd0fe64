// Adding codes to the lists of a Grouping index in HBM (ivfhnsw_gpu_append_grouping / ivfhnsw_gpu_add_groups, DESIGN.md
// 3.12).  A Grouping list is nsubc sub-groups laid end to end (IndexIVF_HNSW_Grouping.cpp:127-155), so a list does not
// only grow at its end as an IVFADC list does (kernels_append.hip): it grows at the end of each of its sub-groups.  Old
// row `within` of sub-group s of list c moves from loff[c] + pre_old[c][s] + within to lstart[c] + pre_new[c][s] + within,
// and the new rows of (c, s) follow it in arrival order.  One out-of-place merge builds the new CSR:
//   count    cnt[c] += 1 and sizes2[c][s] += 1 per batch row (global atomics; sizes2 starts as a copy of the sizes table,
//            so it ends as the new table); a list id >= nc or a sub-group id >= nsubc raises *status and is not counted
//   scan     own / nstart / lstart exactly as the IVFADC append (launch_append_tables), then goff' / loff' and the tiles'
//            first lists (launch_append_layout)
//   prefix   for every TOUCHED list (nstart[c + 1] > nstart[c]) the exclusive prefix sums of its old and of its new
//            sub-group sizes, one wavefront per list: pre_old[c][s], pre_new[c][s].  Untouched lists cost one load here
//   merge    destination-tiled like append_merge_kernel (append_tile.h).  A row of an untouched list takes the plain path
//            (source = loff[c] + off); a row of a touched list finds its sub-group by one binary search over the list's
//            nsubc new prefix sums, which the tile holds in LDS when they fit (log2 nsubc LDS reads per row)
//   scatter  row p of the batch sorted stably by (list, sub-group) -- two LSD radix sorts, by sub-group and then by list,
//            as nc * nsubc can exceed 2^32 -- goes to lstart[c] + pre_old[c][s] + old_size[c][s] + (p - nstart[c]): behind
//            the old rows of sub-groups <= s and every new row sorted before it in the list
// and for add_groups the table rows of the groups: nn_centroid_idxs, alpha, inter-centroid distances (given, or computed
// in the reference's float order, IndexIVF_HNSW_Grouping.cpp:620-631).
#include "ivfhnsw_kernels.h"
#include "device_common.h"
#include "append_tile.h"

namespace ivfhnsw_gpu_impl {

namespace {

__global__ __launch_bounds__(256) void grouping_count_kernel(const uint32_t *__restrict__ list_idx, const uint32_t *__restrict__ sub_idx,
                                                             size_t n, uint32_t nc, uint32_t nsubc, uint32_t *__restrict__ cnt,
                                                             uint32_t *__restrict__ sizes2, uint32_t *__restrict__ status)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const uint32_t c = list_idx[i], s = sub_idx[i];
    if (c >= nc || s >= nsubc) {
        *status = 1u;
    } else if (cnt) {
        atomicAdd(cnt + c, 1u);
        atomicAdd(sizes2 + (size_t)c * nsubc + s, 1u);
    }
}

// one wavefront per list; lists the batch does not touch are left alone (nobody reads their prefix rows)
__global__ __launch_bounds__(256) void grouping_prefix_kernel(const uint32_t *__restrict__ nstart, const uint32_t *__restrict__ sizes,
                                                              const uint32_t *__restrict__ sizes2, uint32_t *__restrict__ pre_old,
                                                              uint32_t *__restrict__ pre_new, uint32_t nc, uint32_t nsubc)
{
    const int lane = threadIdx.x & 63;
    const size_t c = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (c >= nc || nstart[c + 1] == nstart[c])
        return;
    const size_t row = c * nsubc;
    uint32_t run_old = 0, run_new = 0;
    for (uint32_t s0 = 0; s0 < nsubc; s0 += 64) {
        const uint32_t s = s0 + lane;
        const uint32_t vo = s < nsubc ? sizes[row + s] : 0u, vn = s < nsubc ? sizes2[row + s] : 0u;
        uint32_t io = vo, in = vn;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t yo = __shfl_up(io, o), yn = __shfl_up(in, o);
            if (lane >= o) {
                io += yo;
                in += yn;
            }
        }
        if (s < nsubc) {
            pre_old[row + s] = run_old + io - vo;
            pre_new[row + s] = run_new + in - vn;
        }
        run_old += __shfl(io, 63);
        run_new += __shfl(in, 63);
    }
}

constexpr uint32_t kPrefixCache = 1024; // prefix sums per table a tile keeps in LDS (16 lists at nsubc 64)

// the source row of row `off` of touched list c: pn / po = the list's nsubc new / old prefix sums, old_len its old length
__device__ __forceinline__ uint32_t grouping_source(const uint32_t *pn, const uint32_t *po, uint32_t nsubc, uint32_t off,
                                                    uint32_t old_len, uint32_t loff_c)
{
    // the largest s with pn[s] <= off: the sub-group that holds row off (it is not empty, as the next prefix lies above)
    const uint32_t s = list_of_row(pn, 0u, nsubc - 1, off);
    const uint32_t within = off - pn[s];
    const uint32_t old_size = (s + 1 < nsubc ? po[s + 1] : old_len) - po[s];
    return within < old_size ? loff_c + po[s] + within : kSkip;
}

// append_merge_kernel with the sub-group step for the lists the batch touches.  A tile whose lists' prefix sums fit
// kPrefixCache (the rule at the metric's shape: two to four lists of ~1000 rows per tile) loads them into LDS with
// coalesced, independent loads first, so that a row's search runs at LDS latency; a tile over many short lists searches in
// global memory.
__global__ __launch_bounds__(256) void grouping_merge_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ loff,
                                                             const uint32_t *__restrict__ nstart, const uint32_t *__restrict__ lstart,
                                                             const uint32_t *__restrict__ tile_first,
                                                             const uint32_t *__restrict__ pre_old, const uint32_t *__restrict__ pre_new,
                                                             uint32_t nsubc, const uint32_t *__restrict__ codes,
                                                             const uint8_t *__restrict__ ncodes, const uint32_t *__restrict__ ids,
                                                             uint32_t *__restrict__ codes2, uint8_t *__restrict__ ncodes2,
                                                             uint32_t *__restrict__ ids2, uint32_t n_local2, uint32_t q)
{
    __shared__ uint32_t s_src[kAppendTileRows];
    __shared__ uint32_t s_pn[kPrefixCache], s_po[kPrefixCache];
    const uint32_t r0 = blockIdx.x * (uint32_t)kAppendTileRows;
    const uint32_t rows = min((uint32_t)kAppendTileRows, n_local2 - r0);
    const uint32_t lo = tile_first[blockIdx.x], hi = tile_first[blockIdx.x + 1];
    const uint32_t cached_words = (uint64_t)(hi - lo + 1) * nsubc <= kPrefixCache ? (hi - lo + 1) * nsubc : 0u;
    for (uint32_t w = threadIdx.x; w < cached_words; w += 256) {
        const uint32_t c = lo + w / nsubc;
        if (nstart[c + 1] != nstart[c]) { // (untouched lists have no prefix rows)
            const size_t g = (size_t)c * nsubc + w % nsubc;
            s_pn[w] = pre_new[g];
            s_po[w] = pre_old[g];
        }
    }
    __syncthreads();
    for (uint32_t j = threadIdx.x; j < rows; j += 256) {
        const uint32_t r = r0 + j;
        const uint32_t c = list_of_row(lstart, lo, hi, r);
        const uint32_t off = r - lstart[c];
        const uint32_t old_len = (uint32_t)(goff[c + 1] - goff[c]);
        uint32_t src;
        if (nstart[c + 1] == nstart[c]) // untouched: the list moves as a whole
            src = off < old_len ? loff[c] + off : kSkip;
        else if (cached_words)
            src = grouping_source(s_pn + (c - lo) * nsubc, s_po + (c - lo) * nsubc, nsubc, off, old_len, loff[c]);
        else
            src = grouping_source(pre_new + (size_t)c * nsubc, pre_old + (size_t)c * nsubc, nsubc, off, old_len, loff[c]);
        s_src[j] = src;
    }
    __syncthreads();
    copy_tile_dwords(codes, codes2 + (size_t)r0 * q, s_src, rows * q, q);
    copy_tile_dwords(ids, ids2 + r0, s_src, rows, 1u);
    copy_tile_norm_codes(ncodes, ncodes2, s_src, r0, rows);
}

// one thread per dword of the new codes, in sorted order: code p of the sorted batch is input row perm[p]
__global__ __launch_bounds__(256) void grouping_scatter_kernel(const uint32_t *__restrict__ perm, const uint32_t *__restrict__ list_idx,
                                                               const uint32_t *__restrict__ sub_idx, const uint32_t *__restrict__ nstart,
                                                               const uint32_t *__restrict__ loff, const uint32_t *__restrict__ lstart,
                                                               const uint32_t *__restrict__ sizes, const uint32_t *__restrict__ pre_old,
                                                               uint32_t nsubc, const uint32_t *__restrict__ new_codes,
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
    const size_t cs = (size_t)c * nsubc + sub_idx[i];
    const size_t row = (size_t)lstart[c] + pre_old[cs] + sizes[cs] + (p - nstart[c]);
    codes2[row * q + k] = new_codes[(size_t)i * q + k];
    if (k == 0) {
        ids2[row] = new_ids[i];
        ncodes2[row] = new_norm[i];
    }
}

// *status (set to 0xffffffff before) = the lowest g whose list already holds codes
__global__ __launch_bounds__(256) void groups_empty_kernel(const uint64_t *__restrict__ goff, const uint32_t *__restrict__ cidx,
                                                           uint32_t ngroups, uint32_t nc, uint32_t *__restrict__ status)
{
    const uint32_t g = blockIdx.x * 256 + threadIdx.x;
    if (g >= ngroups)
        return;
    const uint32_t c = cidx[g];
    if (c < nc && goff[c + 1] != goff[c])
        atomicMin(status, g);
}

// list_idx[p] = the centroid of the group that point p belongs to (off: [G + 1] point offsets of the chunk's groups)
__global__ __launch_bounds__(256) void groups_point_lists_kernel(const unsigned long long *__restrict__ off,
                                                                 const uint32_t *__restrict__ cidx, uint32_t G,
                                                                 uint32_t *__restrict__ list_idx)
{
    const uint32_t g = blockIdx.x;
    const uint32_t c = cidx[g];
    for (unsigned long long p = off[g] + threadIdx.x; p < off[g + 1]; p += 256)
        list_idx[p] = c;
}

// One workgroup per group: the neighbour row always (IndexIVF_HNSW_Grouping.cpp:62); alpha and the inter-centroid row
// only when the group has points (:63-64 returns before them).  inter_src null: row s = the distance from the neighbour
// centroid to the group's centroid in the reference's order (:620-631), a quad of lanes per neighbour.
__global__ __launch_bounds__(256) void groups_rows_kernel(const uint32_t *__restrict__ cidx, const unsigned long long *__restrict__ off,
                                                          const uint32_t *__restrict__ nn_src, const float *__restrict__ alpha_src,
                                                          const float *__restrict__ inter_src, const float *__restrict__ vectors,
                                                          int d, uint32_t nsubc, uint32_t *__restrict__ nn_dst,
                                                          float *__restrict__ alpha_dst, float *__restrict__ inter_dst)
{
    extern __shared__ float s_c[];
    const uint32_t g = blockIdx.x;
    const size_t c = cidx[g], src = (size_t)g * nsubc, dst = c * nsubc;
    for (uint32_t s = threadIdx.x; s < nsubc; s += 256)
        nn_dst[dst + s] = nn_src[src + s];
    if (off[g + 1] == off[g])
        return;
    if (threadIdx.x == 0)
        alpha_dst[c] = alpha_src[g];
    if (inter_src) {
        for (uint32_t s = threadIdx.x; s < nsubc; s += 256)
            inter_dst[dst + s] = inter_src[src + s];
        return;
    }
    for (int j = threadIdx.x; j < d; j += 256)
        s_c[j] = vectors[c * d + j];
    __syncthreads();
    const int t = threadIdx.x & 3;
    for (uint32_t s0 = 0; s0 < nsubc; s0 += 64) { // whole quads stay together: the loop bound is uniform
        const uint32_t s = s0 + (threadIdx.x >> 2);
        const uint32_t nn = s < nsubc ? nn_src[src + s] : (uint32_t)c;
        const float v = l2_ref_order_quad(vectors + (size_t)nn * d, s_c, d, t);
        if (s < nsubc && t == 0)
            inter_dst[dst + s] = v;
    }
}

// out[i][:] = table[rows[i]][:] (rows of nsubc words)
__global__ __launch_bounds__(256) void gather_rows_kernel(const uint32_t *__restrict__ table, const uint32_t *__restrict__ rows,
                                                          uint32_t nsubc, uint32_t *__restrict__ out)
{
    const size_t r = rows[blockIdx.x];
    for (uint32_t s = threadIdx.x; s < nsubc; s += 256)
        out[(size_t)blockIdx.x * nsubc + s] = table[r * nsubc + s];
}

inline unsigned blocks_of(size_t n, size_t per) { return (unsigned)((n + per - 1) / per); }

} // namespace

hipError_t launch_grouping_count(hipStream_t s, const uint32_t *list_idx, const uint32_t *sub_idx, size_t n, uint32_t nc,
                                 uint32_t nsubc, uint32_t *cnt, uint32_t *sizes2, uint32_t *status)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(grouping_count_kernel, dim3(blocks_of(n, 256)), dim3(256), 0, s, list_idx, sub_idx, n, nc, nsubc, cnt,
                       sizes2, status);
    return hipGetLastError();
}

hipError_t launch_grouping_prefix(hipStream_t s, const uint32_t *nstart, const uint32_t *sizes, const uint32_t *sizes2,
                                  uint32_t *pre_old, uint32_t *pre_new, uint32_t nc, uint32_t nsubc)
{
    hipLaunchKernelGGL(grouping_prefix_kernel, dim3(blocks_of(nc, 4)), dim3(256), 0, s, nstart, sizes, sizes2, pre_old, pre_new,
                       nc, nsubc);
    return hipGetLastError();
}

hipError_t launch_grouping_merge(hipStream_t s, const IvfTables &t, const uint32_t *nstart, const uint32_t *lstart,
                                 const uint32_t *tile_first, const uint32_t *pre_old, const uint32_t *pre_new,
                                 uint32_t nsubc, const NewLists &nl)
{
    if (nl.n_local == 0)
        return hipSuccess;
    if (nl.n_local >= 0xffffffffull || t.M % 4 || nsubc == 0)
        return hipErrorInvalidValue;
    const uint32_t ntiles = blocks_of(nl.n_local, kAppendTileRows);
    hipLaunchKernelGGL(grouping_merge_kernel, dim3(ntiles), dim3(256), 0, s, t.goff, t.loff, nstart, lstart, tile_first,
                       pre_old, pre_new, nsubc, reinterpret_cast<const uint32_t *>(t.codes), t.norm_codes, t.ids,
                       reinterpret_cast<uint32_t *>(nl.codes), nl.ncodes, nl.ids, (uint32_t)nl.n_local, (uint32_t)(t.M / 4));
    return hipGetLastError();
}

hipError_t launch_grouping_scatter(hipStream_t s, const IvfTables &t, const uint32_t *perm, const uint32_t *list_idx,
                                   const uint32_t *sub_idx, size_t n, const uint32_t *nstart, const uint32_t *lstart,
                                   const uint32_t *sizes, const uint32_t *pre_old, uint32_t nsubc, const uint8_t *codes,
                                   const uint8_t *norm_codes, const uint32_t *ids, const NewLists &nl)
{
    if (n == 0)
        return hipSuccess;
    const uint32_t q = (uint32_t)(t.M / 4);
    hipLaunchKernelGGL(grouping_scatter_kernel, dim3(blocks_of(n * q, 256)), dim3(256), 0, s, perm, list_idx, sub_idx, nstart,
                       t.loff, lstart, sizes, pre_old, nsubc, reinterpret_cast<const uint32_t *>(codes), norm_codes, ids,
                       reinterpret_cast<uint32_t *>(nl.codes), nl.ncodes, nl.ids, n, q);
    return hipGetLastError();
}

hipError_t launch_groups_empty(hipStream_t s, const uint64_t *goff, const uint32_t *cidx, size_t ngroups, uint32_t nc,
                               uint32_t *status)
{
    if (ngroups == 0)
        return hipSuccess;
    hipLaunchKernelGGL(groups_empty_kernel, dim3(blocks_of(ngroups, 256)), dim3(256), 0, s, goff, cidx, (uint32_t)ngroups, nc,
                       status);
    return hipGetLastError();
}

hipError_t launch_groups_point_lists(hipStream_t s, const unsigned long long *off, const uint32_t *cidx, size_t G,
                                     uint32_t *list_idx)
{
    if (G == 0)
        return hipSuccess;
    hipLaunchKernelGGL(groups_point_lists_kernel, dim3((unsigned)G), dim3(256), 0, s, off, cidx, (uint32_t)G, list_idx);
    return hipGetLastError();
}

hipError_t launch_groups_rows(hipStream_t s, const uint32_t *cidx, const unsigned long long *off, const uint32_t *nn_src,
                              const float *alpha_src, const float *inter_src, const float *vectors, int d, uint32_t nsubc,
                              size_t G, uint32_t *nn_dst, float *alpha_dst, float *inter_dst)
{
    if (G == 0)
        return hipSuccess;
    if (!inter_src && (d % 8 || (size_t)d * sizeof(float) > 64 * 1024))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(groups_rows_kernel, dim3((unsigned)G), dim3(256), (size_t)d * sizeof(float), s, cidx, off, nn_src,
                       alpha_src, inter_src, vectors, d, nsubc, nn_dst, alpha_dst, inter_dst);
    return hipGetLastError();
}

hipError_t launch_gather_rows(hipStream_t s, const uint32_t *table, const uint32_t *rows, size_t nrows, uint32_t nsubc,
                              uint32_t *out)
{
    if (nrows == 0)
        return hipSuccess;
    hipLaunchKernelGGL(gather_rows_kernel, dim3((unsigned)nrows), dim3(256), 0, s, table, rows, nsubc, out);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
