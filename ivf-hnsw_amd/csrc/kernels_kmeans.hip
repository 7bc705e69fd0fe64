// Exact Lloyd k-means for the IVF coarse centroids (ivfhnsw_gpu_kmeans).  The reference never learns
// them: its README points to downloaded centroid files, and every driver reads them as -path_centroids
// (tests/test_ivfhnsw_sift1b.cpp, IndexIVF_HNSW::build_quantizer).
//
// The assignment step is ivfhnsw_gpu_knn's k = 1 table (kernels_knn.hip) as it is.  This file holds the rest of an
// iteration, built for nc ~ 10^6 clusters, where lloyd_update_kernel's "every block scans all n points" cannot work:
//   count    cnt[c] by global atomics, and the objective's per-block partial sums (fixed tree order, double)
//   members  the point ids sorted by cluster, STABLY: an LSD radix sort on the assignment, 8 bits per pass, whose input
//            is the identity permutation.  So each cluster's members come out in ascending point order -- the order the
//            float sums below are taken in, which is the contract.  Clusters of any size take the same path.
//   means    one wavefront per cluster, lane l owns components 2l and 2l + 1, the member rows gathered in order:
//            S = ((0 + x0) + x1) + ...   (__fadd_rn), mean = S / (float)cnt (__fdiv_rn); an empty cluster keeps its row
//   split    the (ci, cj) pairs the host picked (faiss's split_clusters, deterministic), applied strictly in order
#include "ivfhnsw_kernels.h"
#include "update_steps.h"

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int kTileRounds = kKmeansTile / 256; // a 256-thread block takes its tile in rounds of 256 consecutive points

// cnt[assign[i]] += 1; part[block] = sum of the tile's dist in double (tree order fixed); an id >= nc (no finite
// distance: NaN or inf in the input) raises *status and is not counted
__global__ __launch_bounds__(256) void kmeans_count_kernel(const uint32_t *__restrict__ assign, const float *__restrict__ dist,
                                                           size_t n, uint32_t nc, uint32_t *__restrict__ cnt,
                                                           double *__restrict__ part, uint32_t *__restrict__ status)
{
    __shared__ double s[256];
    const int t = threadIdx.x;
    const size_t i0 = (size_t)blockIdx.x * kKmeansTile;
    double acc = 0.0;
    for (int r = 0; r < kTileRounds; r++) {
        const size_t i = i0 + (size_t)r * 256 + t;
        if (i < n) {
            const uint32_t a = assign[i];
            if (a < nc)
                atomicAdd(cnt + a, 1u);
            else
                *status = 1u;
            acc += (double)dist[i];
        }
    }
    s[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o)
            s[t] += s[t + o];
        __syncthreads();
    }
    if (t == 0)
        part[blockIdx.x] = s[0];
}

// out[i] = in[0] + ... + in[i - 1] (exclusive; in == out allowed).  One workgroup walks the array in chunks of 1024
// with a carried prefix: the arrays are nc counts or 256 x (n / 4096) histogram cells, a few microseconds per chunk.
__global__ __launch_bounds__(1024) void scan_u32_kernel(const uint32_t *in, uint32_t *out, size_t len)
{
    __shared__ uint32_t s_w[16];
    uint32_t carry = 0; // the sum of the chunks before, kept by every thread
    for (size_t c0 = 0; c0 < len; c0 += 1024) { // every thread walks every chunk: block_excl_scan sees whole wavefronts
        const size_t i = c0 + threadIdx.x;
        const uint32_t v = i < len ? in[i] : 0u;
        uint32_t total;
        const uint32_t excl = block_excl_scan<16>(v, s_w, total);
        if (i < len)
            out[i] = carry + excl;
        carry += total;
    }
}

// the element at position i of the pass's input (the identity for the first pass; the clamp only bounds the key read)
__device__ __forceinline__ uint32_t sort_id(const uint32_t *in_ids, size_t i, size_t n)
{
    return in_ids ? (uint32_t)min((size_t)in_ids[i], n - 1) : (uint32_t)i;
}

// hist[digit * nblocks + block] = elements of the block's tile whose key digit ((key >> shift) & 255) is `digit`
__global__ __launch_bounds__(256) void radix_hist_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ in_ids,
                                                         size_t n, int shift, uint32_t *__restrict__ hist, uint32_t nblocks)
{
    __shared__ uint32_t h[256];
    const int t = threadIdx.x;
    h[t] = 0;
    __syncthreads();
    const size_t i0 = (size_t)blockIdx.x * kKmeansTile;
    for (int r = 0; r < kTileRounds; r++) {
        const size_t i = i0 + (size_t)r * 256 + t;
        if (i < n)
            atomicAdd(&h[(keys[sort_id(in_ids, i, n)] >> shift) & 255u], 1u);
    }
    __syncthreads();
    hist[(size_t)t * nblocks + blockIdx.x] = h[t];
}

// Stable scatter: an element's place = the exclusive offset of (digit, block) + the elements of the same digit before it
// in the tile.  The tile goes in rounds of 256 consecutive elements; inside a round, the rank among the wave's lanes
// comes from eight ballots (the lanes whose digit matches), the waves before it from a per-wave digit count in LDS.
__global__ __launch_bounds__(256) void radix_scatter_kernel(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ in_ids,
                                                            uint32_t *__restrict__ out_ids, size_t n, int shift,
                                                            const uint32_t *__restrict__ offs, uint32_t nblocks)
{
    __shared__ uint32_t s_base[256];
    __shared__ uint32_t s_wcnt[4][256];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    s_base[t] = offs[(size_t)t * nblocks + blockIdx.x];
    const size_t i0 = (size_t)blockIdx.x * kKmeansTile;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (int r = 0; r < kTileRounds; r++) {
#pragma unroll
        for (int w = 0; w < 4; w++)
            s_wcnt[w][t] = 0;
        __syncthreads();
        const size_t i = i0 + (size_t)r * 256 + t;
        const bool valid = i < n;
        const uint32_t id = valid ? sort_id(in_ids, i, n) : 0u;
        const uint32_t dg = valid ? (keys[id] >> shift) & 255u : 0u;
        unsigned long long peers = __ballot(valid);
#pragma unroll
        for (int b = 0; b < 8; b++) {
            const bool bit = (dg >> b) & 1u;
            const unsigned long long m = __ballot(bit);
            peers &= bit ? m : ~m;
        }
        const uint32_t rank = (uint32_t)__popcll(peers & below);
        if (valid && rank == 0)
            s_wcnt[wave][dg] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = s_base[dg] + rank;
            for (int w = 0; w < wave; w++)
                pos += s_wcnt[w][dg];
            if (pos < n) // always, as the histogram counted these very digits
                out_ids[pos] = id;
        }
        __syncthreads(); // every lane has read s_base
        s_base[t] += s_wcnt[0][t] + s_wcnt[1][t] + s_wcnt[2][t] + s_wcnt[3][t];
        __syncthreads();
    }
}

// One wavefront per cluster: the member rows in ascending point order (64 ids per coalesced load, then four rows'
// loads in flight ahead of their adds), lane l summing components 2l and 2l + 1.
__global__ __launch_bounds__(256) void kmeans_mean_kernel(const float *__restrict__ x, const uint32_t *__restrict__ members,
                                                          const uint32_t *__restrict__ start, const uint32_t *__restrict__ cnt,
                                                          float *__restrict__ c, uint32_t nc, int d, uint32_t n)
{
    const int lane = threadIdx.x & 63;
    const size_t cl = (size_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (cl >= nc)
        return;
    const uint32_t m = cnt[cl];
    if (m == 0)
        return;
    const uint32_t s0 = start[cl];
    const bool on = 2 * lane < d;
    const int col = on ? 2 * lane : 0;
    float a0 = 0.f, a1 = 0.f;
    for (uint32_t j0 = 0; j0 < m; j0 += 64) {
        const uint32_t my = j0 + lane < m ? members[(size_t)s0 + j0 + lane] : 0u;
        const int len = (int)min(64u, m - j0);
        int j = 0;
        for (; j + 4 <= len; j += 4) {
            float2 v[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const uint32_t id = min(__shfl(my, j + u), n - 1u); // (member ids are < n; the clamp keeps it so)
                v[u] = *reinterpret_cast<const float2 *>(x + (size_t)id * d + col);
            }
#pragma unroll
            for (int u = 0; u < 4; u++) {
                a0 = __fadd_rn(a0, v[u].x);
                a1 = __fadd_rn(a1, v[u].y);
            }
        }
        for (; j < len; j++) {
            const uint32_t id = min(__shfl(my, j), n - 1u);
            const float2 v = *reinterpret_cast<const float2 *>(x + (size_t)id * d + col);
            a0 = __fadd_rn(a0, v.x);
            a1 = __fadd_rn(a1, v.y);
        }
    }
    if (on) {
        const float fm = (float)m;
        *reinterpret_cast<float2 *>(c + cl * d + col) = make_float2(__fdiv_rn(a0, fm), __fdiv_rn(a1, fm));
    }
}

// faiss's split_clusters with the choice made: for each (ci, cj) IN ORDER, row ci = row cj, then component j of ci is
// scaled by 1 + EPS and of cj by 1 - EPS for even j, the other way round for odd j (EPS = 1/1024).  Thread j owns
// component j of every row, so a pair that reads a row an earlier pair wrote reads that thread's own store.
__global__ __launch_bounds__(128) void kmeans_split_kernel(float *__restrict__ c, const uint32_t *__restrict__ pairs,
                                                           uint32_t npairs, int d)
{
    const int j = threadIdx.x;
    if (j >= d)
        return;
    const float up = 1.0f + 1.0f / 1024.0f, dn = 1.0f - 1.0f / 1024.0f;
    const float fi = (j & 1) ? dn : up, fj = (j & 1) ? up : dn;
    for (uint32_t p = 0; p < npairs; p++) {
        const size_t ci = pairs[2 * (size_t)p], cj = pairs[2 * (size_t)p + 1];
        const float v = c[cj * d + j];
        c[ci * d + j] = __fmul_rn(v, fi);
        c[cj * d + j] = __fmul_rn(v, fj);
    }
}

} // namespace

hipError_t launch_kmeans_count(hipStream_t s, const uint32_t *assign, const float *dist, size_t n, uint32_t nc,
                               uint32_t *cnt, double *part, uint32_t *status)
{
    if (n == 0)
        return hipSuccess;
    const size_t nblocks = (n + kKmeansTile - 1) / kKmeansTile;
    hipLaunchKernelGGL(kmeans_count_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, assign, dist, n, nc, cnt, part, status);
    return hipGetLastError();
}

hipError_t launch_scan_u32(hipStream_t s, const uint32_t *in, uint32_t *out, size_t len)
{
    if (len == 0)
        return hipSuccess;
    hipLaunchKernelGGL(scan_u32_kernel, dim3(1), dim3(1024), 0, s, in, out, len);
    return hipGetLastError();
}

hipError_t launch_sort_by_key(hipStream_t s, const uint32_t *keys, size_t n, int key_bits, uint32_t *ids_a, uint32_t *ids_b,
                              uint32_t *hist, uint32_t **sorted)
{
    return launch_sort_by_key_from(s, keys, n, key_bits, nullptr, ids_a, ids_b, hist, sorted);
}

hipError_t launch_sort_by_key_from(hipStream_t s, const uint32_t *keys, size_t n, int key_bits, const uint32_t *start,
                                   uint32_t *ids_a, uint32_t *ids_b, uint32_t *hist, uint32_t **sorted)
{
    const size_t nblocks = (n + kKmeansTile - 1) / kKmeansTile;
    const int passes = key_bits <= 8 ? 1 : (key_bits + 7) / 8;
    const uint32_t *in = start; // null: pass 0 reads the identity permutation
    uint32_t *out = start == ids_a ? ids_b : ids_a;
    for (int p = 0; p < passes; p++) {
        hipLaunchKernelGGL(radix_hist_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, keys, in, n, 8 * p, hist,
                           (uint32_t)nblocks);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
        if (hipError_t e = launch_scan_u32(s, hist, hist, 256 * nblocks); e != hipSuccess)
            return e;
        hipLaunchKernelGGL(radix_scatter_kernel, dim3((unsigned)nblocks), dim3(256), 0, s, keys, in, out, n, 8 * p, hist,
                           (uint32_t)nblocks);
        if (hipError_t e = hipGetLastError(); e != hipSuccess)
            return e;
        in = out;
        out = out == ids_a ? ids_b : ids_a;
    }
    *sorted = const_cast<uint32_t *>(in);
    return hipSuccess;
}

hipError_t launch_kmeans_means(hipStream_t s, const float *x, size_t n, const uint32_t *members, const uint32_t *start,
                               const uint32_t *cnt, float *c, size_t nc, int d)
{
    if (nc == 0 || n == 0)
        return hipSuccess;
    if (n > 0xffffffffull || d < 2 || d > 128 || (d & 1))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmeans_mean_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, s, x, members, start, cnt, c,
                       (uint32_t)nc, d, (uint32_t)n);
    return hipGetLastError();
}

hipError_t launch_kmeans_split(hipStream_t s, float *c, const uint32_t *pairs, size_t npairs, int d)
{
    if (npairs == 0)
        return hipSuccess;
    if (d < 1 || d > 128)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(kmeans_split_kernel, dim3(1), dim3(128), 0, s, c, pairs, (uint32_t)npairs, d);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
