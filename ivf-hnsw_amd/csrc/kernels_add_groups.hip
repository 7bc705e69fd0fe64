// Adding codes to the lists of a Grouping index in HBM (ivfhnsw_gpu_append_grouping / ivfhnsw_gpu_add_groups, DESIGN.md
// 3.12).  A Grouping list is nsubc sub-groups laid end to end (IndexIVF_HNSW_Grouping.cpp:127-155), so a list does not
// only grow at its end as an IVFADC list does (kernels_append.hip): it grows at the end of each of its sub-groups.  Old
// row `within` of sub-group s of list c moves from loff[c] + pre_old[c][s] + within to lstart[c] + pre_new[c][s] + within,
// and the new rows of (c, s) follow it in arrival order.  One out-of-place merge builds the new CSR with the append's
// kernels (kernels_append.hip: count, scans, layout, append_merge_kernel<true>, append_scatter_kernel<true>; the sub-group
// tables travel as SubGroups), after two stable radix sorts of the batch, by sub-group and then by list (nc * nsubc can
// exceed 2^32), and one kernel of this file:
//   prefix   for every TOUCHED list (nstart[c + 1] > nstart[c]) the exclusive prefix sums of its old and of its new
//            sub-group sizes, one wavefront per list: pre_old[c][s], pre_new[c][s].  Untouched lists cost one load
// and for add_groups the table rows of the groups: nn_centroid_idxs, alpha, inter-centroid distances (given, or computed
// in the reference's float order, IndexIVF_HNSW_Grouping.cpp:620-631).
#include "ivfhnsw_kernels.h"
#include "update_steps.h"

namespace ivfhnsw_gpu_impl {

namespace {

// one wavefront per list; lists the batch does not touch are left alone (nobody reads their prefix rows).  The exit is
// wavefront-uniform and lanes past nsubc scan a 0, so wave_incl_scan sees all 64 lanes
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
        const uint32_t io = wave_incl_scan(vo, lane), in = wave_incl_scan(vn, lane);
        if (s < nsubc) {
            pre_old[row + s] = run_old + io - vo;
            pre_new[row + s] = run_new + in - vn;
        }
        run_old += __shfl(io, 63);
        run_new += __shfl(in, 63);
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

} // namespace

hipError_t launch_grouping_prefix(hipStream_t s, const uint32_t *nstart, const uint32_t *sizes, const uint32_t *sizes2,
                                  uint32_t *pre_old, uint32_t *pre_new, uint32_t nc, uint32_t nsubc)
{
    hipLaunchKernelGGL(grouping_prefix_kernel, dim3(blocks_of(nc, 4)), dim3(256), 0, s, nstart, sizes, sizes2, pre_old, pre_new,
                       nc, nsubc);
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
