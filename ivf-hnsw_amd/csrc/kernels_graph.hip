// ivfhnsw_gpu_build_graph_dev: hnswlib's addPoint loop (hnswlib/hnswalg.cpp:212-225) for all nodes at once, on the device.
//
// The one deviation from the reference: a new node's link candidates are its EXACT ncand nearest among the nodes
// inserted before it -- one triangular sweep of the MFMA neighbour-table kernel (kernels_knn.hip, IVFHNSW_KNN_EARLIER)
// -- instead of the efConstruction results of a greedy search of the graph built so far (hnswalg.cpp:221).  With that,
// a node's forward links no longer depend on the state of the graph, so the serial insertion loop unrolls exactly:
//   A. forward links of every node c, independently: getNeighborsByHeuristic over its candidates down to M
//      (hnswalg.cpp:110-146; distances by fstdistfunc's order, :326-357), stored farthest first (:153-170);
//   B. reverse lists: for every node t the later nodes c that chose t, ascending c (= the order the serial loop meets
//      them): a stable radix sort (kernels_kmeans.hip) of the link slots c * M + i by the node they name, capi_build.cpp;
//   C. the fold of mutuallyConnectNewElement's second half over t's reverse list, independently per t: append while t has
//      room, else shrink t's maxM + 1 candidates with the same heuristic (:171-209).
// The result is what the serial loop leaves, link for link (tests/test_gpu_graph_build*.py against the oracle's serial
// restatement).
//
// A and C take one node per wavefront (a workgroup of 64 lanes).  The rows a node works on are staged in LDS, padded to
// d + 8 floats so that the eight rows of one distance pass start eight banks apart; every distance is
// l2_ref_order_oct's: eight lanes per row, lane l owning the reference's accumulator l, the eight sums added left to
// right.  The table's MFMA distances are never read.  The heuristic's early `break` (hnswalg.cpp:131-136) only decides
// whether some kept neighbour is closer to the candidate than the node is, so testing all kept neighbours of a candidate
// across lanes is exact.  No float atomics; a node's result depends on nothing but the rows, so neither on the grid.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

#include <algorithm>

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int kRowPad = 8;
constexpr int kMaxCand = 80; // ivfhnsw_gpu_knn's k limit
constexpr int kMaxLinks = 64;
constexpr uint32_t kNoCand = 0xffffffffu;

// (a before b) in the order resultSet pops in: ascending distance, larger id first among equal distances
__device__ __forceinline__ bool pops_before(float da, uint32_t ia, float db, uint32_t ib)
{
    return da < db || (da == db && ia > ib);
}
// (a before b) in the order the links are stored in: farthest first, larger id first among equals
__device__ __forceinline__ bool stored_before(float da, uint32_t ia, float db, uint32_t ib)
{
    return da > db || (da == db && ia > ib);
}

// rows s_ids[0 .. nrows - 1] of x into LDS, row r to dst(r); eight float4 loads per lane in flight
template <class Dst>
__device__ __forceinline__ void stage_rows(const float *__restrict__ x, int d, int nrows, const uint32_t *s_ids, int lane, Dst dst)
{
    const int q4 = d >> 2, total = nrows * q4;
    for (int f0 = 0; f0 < total; f0 += 64 * 8) {
        float4 v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int f = f0 + u * 64 + lane;
            if (f < total) {
                const int r = f / q4;
                v[u] = reinterpret_cast<const float4 *>(x + (size_t)s_ids[r] * d)[f - r * q4];
            }
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const int f = f0 + u * 64 + lane;
            if (f < total) {
                const int r = f / q4;
                reinterpret_cast<float4 *>(dst(r))[f - r * q4] = v[u];
            }
        }
    }
}

// A. forward links.  LDS: [ncand + 1] rows (the last is the node's own).
__global__ __launch_bounds__(64) void graph_forward_kernel(const float *__restrict__ x, const uint32_t *__restrict__ table,
                                                           uint32_t n, int d, int M, int ncand, uint32_t *__restrict__ fwd,
                                                           uint8_t *__restrict__ fcnt, uint32_t *__restrict__ deg)
{
    extern __shared__ __align__(16) float s_rows[];
    __shared__ uint32_t s_id[kMaxCand + 1];
    __shared__ float s_dist[kMaxCand];
    __shared__ int s_order[kMaxCand];
    __shared__ int s_kept[kMaxLinks];
    const int lane = threadIdx.x, grp = lane >> 3, t8 = lane & 7;
    const int stride = d + kRowPad;
    for (int i = lane; i < kMaxCand; i += 64)
        s_order[i] = 0;
    for (uint32_t c = blockIdx.x; c < n; c += gridDim.x) {
        __syncthreads(); // the node before is done with the LDS
        // the candidates: the row up to its first empty slot (an id that is no earlier node ends it as well)
        const uint32_t *row = table + (size_t)c * ncand;
        const uint32_t id0 = lane < ncand ? row[lane] : kNoCand;
        const uint32_t id1 = lane + 64 < ncand ? row[lane + 64] : kNoCand;
        const unsigned long long end0 = __ballot(id0 >= c), end1 = __ballot(id1 >= c);
        const int nc = end0 ? __builtin_ctzll(end0) : 64 + (end1 ? __builtin_ctzll(end1) : 0);
        if (lane < nc)
            s_id[lane] = id0;
        if (lane + 64 < nc)
            s_id[lane + 64] = id1;
        if (lane == 0)
            s_id[nc] = c;
        __syncthreads();
        float *self = s_rows + ncand * stride;
        stage_rows(x, d, nc + 1, s_id, lane, [&](int r) { return r < nc ? s_rows + r * stride : self; });
        __syncthreads();
        for (int r0 = 0; r0 < nc; r0 += 8) {
            const int r = min(r0 + grp, nc - 1);
            const float dist = l2_ref_order_oct(s_rows + r * stride, self, d, t8);
            if (t8 == 0 && r0 + grp < nc)
                s_dist[r] = dist;
        }
        __syncthreads();
        for (int r = lane; r < nc; r += 64) {
            const float dr = s_dist[r];
            const uint32_t ir = s_id[r];
            int rank = 0;
            for (int s = 0; s < nc; s++)
                rank += pops_before(s_dist[s], s_id[s], dr, ir) ? 1 : 0;
            s_order[rank] = r;
        }
        __syncthreads();
        int nk = 0;
        if (nc >= M) {
            for (int i = 0; i < nc && nk < M; i++) {
                const int cs = s_order[i];
                const float dc = s_dist[cs];
                const float *crow = s_rows + cs * stride;
                bool closer = false; // some kept neighbour is closer to the candidate than the node is
                for (int j0 = 0; j0 < nk && !closer; j0 += 8) {
                    const int j = min(j0 + grp, nk - 1);
                    const float pd = l2_ref_order_oct(s_rows + s_kept[j] * stride, crow, d, t8);
                    closer = __ballot(t8 == 0 && pd < dc) != 0ull;
                }
                if (!closer) {
                    if (lane == 0)
                        s_kept[nk] = cs;
                    nk++;
                    __syncthreads();
                }
            }
        } else { // fewer than M candidates: all kept, unpruned (hnswalg.cpp:112-113)
            nk = nc;
            if (lane < nc)
                s_kept[lane] = s_order[lane];
        }
        __syncthreads();
        uint32_t *out = fwd + (size_t)c * M;
        if (lane < nk) {
            const int me = s_kept[lane];
            const float dm = s_dist[me];
            const uint32_t im = s_id[me];
            int rank = 0;
            for (int s = 0; s < nk; s++) {
                const int o = s_kept[s];
                rank += stored_before(s_dist[o], s_id[o], dm, im) ? 1 : 0;
            }
            out[rank] = im;
            atomicAdd(deg + im, 1u);
        }
        if (lane >= nk && lane < M)
            out[lane] = n; // no link: sorts behind every node
        if (lane == 0)
            fcnt[c] = (uint8_t)nk;
    }
}

// the node in LDS slot a against t's cnt live links (s_list) and t itself: a row and a column of the pair table, and
// its distance to t
__device__ __forceinline__ void fold_place(const float *s_rows, const float *s_self, float *s_pair, float *s_dist,
                                           const int *s_list, int a, int cnt, int S, int stride, int d, int grp, int t8)
{
    const float *arow = s_rows + a * stride;
    for (int j0 = 0; j0 <= cnt; j0 += 8) {
        const int j = min(j0 + grp, cnt);
        const int sl = j < cnt ? s_list[j] : -1;
        const float pd = l2_ref_order_oct(sl >= 0 ? s_rows + sl * stride : s_self, arow, d, t8);
        if (t8 == 0 && j0 + grp <= cnt) {
            if (sl >= 0) {
                s_pair[a * S + sl] = pd;
                s_pair[sl * S + a] = pd;
            } else {
                s_dist[a] = pd;
            }
        }
    }
    __syncthreads();
}

// C. the fold.  pairs: the link slots c * M + i sorted by the node they name, stably; roff [n + 1]: where node t's run
// starts.  LDS: maxM + 1 slots of rows (t's live links and the arriving node), t's own row, and the [S][S] distances
// between slots -- pure functions of the rows, computed once when a node arrives and kept while it stays.
__global__ __launch_bounds__(64) void graph_fold_kernel(const float *__restrict__ x, const uint32_t *__restrict__ fwd,
                                                        const uint8_t *__restrict__ fcnt, const uint32_t *__restrict__ roff,
                                                        const uint32_t *__restrict__ pairs, uint32_t n, int d, int M, int maxM,
                                                        uint8_t *__restrict__ counts, uint32_t *__restrict__ links,
                                                        uint32_t *__restrict__ longest)
{
    extern __shared__ __align__(16) float s_rows[];
    __shared__ uint32_t s_id[kMaxLinks + 1];
    __shared__ float s_dist[kMaxLinks + 1];
    __shared__ int s_list[kMaxLinks + 1];
    __shared__ int s_order[kMaxLinks + 1];
    const int lane = threadIdx.x, grp = lane >> 3, t8 = lane & 7;
    const int S = maxM + 1, stride = d + kRowPad, q4 = d >> 2;
    float *s_self = s_rows + S * stride;
    float *s_pair = s_self + stride;
    for (int i = lane; i <= kMaxLinks; i += 64) {
        s_list[i] = 0;
        s_order[i] = 0;
    }
    for (uint32_t t = blockIdx.x; t < n; t += gridDim.x) {
        const int cnt0 = min((int)fcnt[t], M);
        const uint32_t r0 = roff[t];
        const uint32_t rlen = roff[t + 1] - r0;
        const uint32_t *mine = fwd + (size_t)t * M;
        uint32_t *out = links + (size_t)t * maxM;
        if (lane == 0 && rlen)
            atomicMax(longest, rlen);
        if ((uint64_t)cnt0 + rlen <= (uint64_t)maxM) { // t never shrinks: its forward links, then the later nodes in order
            if (lane < maxM) {
                uint32_t v = 0;
                if (lane < cnt0)
                    v = mine[lane];
                else if ((uint32_t)(lane - cnt0) < rlen)
                    v = pairs[r0 + (uint32_t)(lane - cnt0)] / (uint32_t)M;
                out[lane] = v;
            }
            if (lane == 0)
                counts[t] = (uint8_t)(cnt0 + (int)rlen);
            continue;
        }
        __syncthreads(); // the node before is done with the LDS
        if (lane < cnt0) {
            s_id[lane] = min(mine[lane], n - 1u);
            s_list[lane] = lane;
        }
        if (lane == 0)
            s_id[cnt0] = t;
        __syncthreads();
        stage_rows(x, d, cnt0 + 1, s_id, lane, [&](int r) { return r < cnt0 ? s_rows + r * stride : s_self; });
        __syncthreads();
        unsigned long long live = 0ull; // slots 0..63 in use; slot 64 (maxM = 64 only) is live64
        bool live64 = false;
        int cnt = 0;
        for (; cnt < cnt0; cnt++) {
            fold_place(s_rows, s_self, s_pair, s_dist, s_list, cnt, cnt, S, stride, d, grp, t8);
            live |= 1ull << cnt;
        }
        // the arriving rows are fetched one step ahead, their ids two
        const uint32_t Mu = (uint32_t)M;
        uint32_t id_next = min(pairs[r0] / Mu, n - 1u);
        uint32_t id_after = rlen > 1 ? min(pairs[r0 + 1] / Mu, n - 1u) : 0u;
        float4 row_next = make_float4(0.f, 0.f, 0.f, 0.f);
        if (lane < q4)
            row_next = reinterpret_cast<const float4 *>(x + (size_t)id_next * d)[lane];
        for (uint32_t k = 0; k < rlen; k++) {
            const uint32_t c = id_next;
            const float4 crow = row_next;
            if (k + 1 < rlen) {
                id_next = id_after;
                if (lane < q4)
                    row_next = reinterpret_cast<const float4 *>(x + (size_t)id_next * d)[lane];
                if (k + 2 < rlen)
                    id_after = min(pairs[r0 + k + 2] / Mu, n - 1u);
            }
            // cnt <= maxM links live in maxM + 1 slots: one is free
            const int a = ~live ? __builtin_ctzll(~live) : 64;
            if (lane < q4)
                reinterpret_cast<float4 *>(s_rows + a * stride)[lane] = crow;
            if (lane == 0) {
                s_id[a] = c;
                s_list[cnt] = a;
            }
            __syncthreads();
            fold_place(s_rows, s_self, s_pair, s_dist, s_list, a, cnt, S, stride, d, grp, t8);
            if (a < 64)
                live |= 1ull << a;
            else
                live64 = true;
            if (cnt < maxM) {
                cnt++;
                continue;
            }
            // getNeighborsByHeuristic over the maxM + 1 nodes of s_list down to maxM
            const int ncd = cnt + 1;
            for (int p = lane; p < ncd; p += 64) {
                const int sp = s_list[p];
                const float dp = s_dist[sp];
                const uint32_t ip = s_id[sp];
                int rank = 0;
                for (int q = 0; q < ncd; q++) {
                    const int sq = s_list[q];
                    rank += pops_before(s_dist[sq], s_id[sq], dp, ip) ? 1 : 0;
                }
                s_order[rank] = sp;
            }
            __syncthreads();
            // near[p]: the earlier positions whose node is closer to position p's node than t is; position 64 (maxM = 64)
            // is lane 0's second word.  Nothing is visited after position 64, so 64 bits name every node that can be kept
            // when another is judged.
            unsigned long long near0 = 0ull, near1 = 0ull;
            for (int p = lane; p < ncd; p += 64) {
                const int sp = s_order[p];
                const float dp = s_dist[sp];
                unsigned long long m = 0ull;
                for (int b = 0; b < p && b < 64; b++)
                    if (s_pair[s_order[b] * S + sp] < dp)
                        m |= 1ull << b;
                if (p < 64)
                    near0 = m;
                else
                    near1 = m;
            }
            unsigned long long kept = 0ull;
            bool kept64 = false;
            int nk = 0;
            for (int p = 0; p < ncd && nk < maxM; p++) {
                const unsigned long long m = p < 64 ? __shfl(near0, p) : __shfl(near1, 0);
                if ((m & kept) == 0ull) {
                    if (p < 64)
                        kept |= 1ull << p;
                    else
                        kept64 = true;
                    nk++;
                }
            }
            // the kept ones, farthest first; the slots of the others are free again
            for (int p = lane; p < ncd; p += 64) {
                if (!(p < 64 ? (kept >> p) & 1ull : kept64))
                    continue;
                const int sp = s_order[p];
                const float dp = s_dist[sp];
                const uint32_t ip = s_id[sp];
                int rank = 0;
                for (int q = 0; q < ncd; q++) {
                    if (!(q < 64 ? (kept >> q) & 1ull : kept64))
                        continue;
                    const int sq = s_order[q];
                    rank += stored_before(s_dist[sq], s_id[sq], dp, ip) ? 1 : 0;
                }
                s_list[rank] = sp;
            }
            for (int p = 0; p < ncd; p++) {
                if (p < 64 ? (kept >> p) & 1ull : kept64)
                    continue;
                const int sl = __builtin_amdgcn_readfirstlane(s_order[p]);
                if (sl < 64)
                    live &= ~(1ull << sl);
                else
                    live64 = false;
            }
            cnt = nk;
            __syncthreads();
        }
        (void)live64; // (slot 64 is only ever handed out when the other 64 are live)
        __syncthreads();
        if (lane < maxM)
            out[lane] = lane < cnt ? s_id[s_list[lane]] : 0u;
        if (lane == 0)
            counts[t] = (uint8_t)cnt;
    }
}

} // namespace

size_t graph_forward_lds_bytes(int d, int ncand) { return (size_t)(ncand + 1) * (d + kRowPad) * sizeof(float); }

size_t graph_fold_lds_bytes(int d, int maxM)
{
    const size_t S = (size_t)maxM + 1;
    return ((S + 1) * (d + kRowPad) + S * S) * sizeof(float);
}

static unsigned graph_grid(size_t n) { return (unsigned)std::min<size_t>(n, (size_t)1 << 22); }

hipError_t launch_graph_forward(hipStream_t s, const float *x, const uint32_t *table, size_t n, int d, int M, int ncand,
                                uint32_t *fwd, uint8_t *fcnt, uint32_t *deg)
{
    if (n == 0)
        return hipSuccess;
    if (n >= 0xffffffffull || d < 16 || d > 128 || (d & 15) || M < 1 || M > kMaxLinks || ncand < M || ncand > kMaxCand)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(graph_forward_kernel, dim3(graph_grid(n)), dim3(64), graph_forward_lds_bytes(d, ncand), s, x, table,
                       (uint32_t)n, d, M, ncand, fwd, fcnt, deg);
    return hipGetLastError();
}

hipError_t launch_graph_fold(hipStream_t s, const float *x, const uint32_t *fwd, const uint8_t *fcnt, const uint32_t *roff,
                             const uint32_t *pairs, size_t n, int d, int M, int maxM, uint8_t *counts, uint32_t *links,
                             uint32_t *longest)
{
    if (n == 0)
        return hipSuccess;
    if (n >= 0xffffffffull || d < 16 || d > 128 || (d & 15) || M < 1 || M > maxM || maxM > kMaxLinks)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(graph_fold_kernel, dim3(graph_grid(n)), dim3(64), graph_fold_lds_bytes(d, maxM), s, x, fwd, fcnt, roff,
                       pairs, (uint32_t)n, d, M, maxM, counts, links, longest);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
