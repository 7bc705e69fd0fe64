// Exact re-rank of search results against the raw uint8 base rows (IndexIVF_HNSW_Grouping::searchDisk,
// IndexIVF_HNSW_Grouping.cpp:365-395: getL2Distance per result, utils.cpp:98-137, then a sort).
//
// Distance = fvec_L2sqr (utils.cpp:22-52, the host library's csrc/host/utils_host.cpp) bit for bit: eight accumulators,
// acc[l] += (q[8b+l] - float(row[8b+l]))^2 for blocks b = 0 .. d/8-1 in order, then ((acc0+acc1)+acc2)+...+acc7, every
// operation rounded to nearest and none fused.  A QUAD of lanes scores one row, lane t owning accumulators 2t and 2t+1
// (the l2_ref_order_quad model, device_common.h).  The store keeps every row permuted for that split (rerank_permute):
// lane t's dims 8j+2t, 8j+2t+1 (j = 0 .. d/8-1) are the d/4 contiguous bytes [t*d/4, (t+1)*d/4), so a quad reads its row
// as one contiguous d-byte piece with 16-byte loads where d % 64 == 0.
//
// One workgroup per query: the quads gather its kc candidate rows (several per quad in flight), the packed keys
// (distance bits << 32 | label) go to LDS, a bitonic sort orders them (unsigned order = (distance, label) because
// distances are non-negative), and the first k are written out.  Labels outside [0, n) are empty slots: never read.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

#include <float.h>

namespace ivfhnsw_gpu_impl {

constexpr int RR_THREADS_MAX = 256;
constexpr unsigned long long RR_EMPTY = ~0ull; // sorts after every real key (no distance has the bits 0xffffffff: NaN)

// ---- upload: rows in file order -> the store's per-quad layout --------------------------------------------------------
// One dword of the stored row per thread: stored byte p of a row (lane t = p / (d/4), i = p % (d/4)) holds dim 8(i/2)+2t+(i%2).
// GATHER: row r of dst is row row_src[r] of src (a negative entry: row 0, a row nobody reads the result of) -- the
// queries of an exact call laid out by its strip plan in the pass that permutes them.
template <bool GATHER>
__global__ void rerank_permute_kernel(const uint8_t *__restrict__ src, size_t src_stride, uint8_t *__restrict__ dst,
                                      size_t count, int d, const int32_t *__restrict__ row_src)
{
    const int S = d >> 2;       // bytes of one lane's slice
    const int wpr = d >> 2;     // dwords per row
    const size_t total = count * (size_t)wpr;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < total; w += (size_t)gridDim.x * blockDim.x) {
        const size_t r = w / wpr;
        const int p = (int)(w - r * wpr) * 4;
        const int t = p / S, i = p - t * S; // i even, and i, i+1, i+2, i+3 lie in the same slice (S % 4 == 0)
        size_t rs = r;
        if constexpr (GATHER)
            rs = (size_t)max(row_src[r], 0);
        const uint8_t *row = src + rs * src_stride;
        const int j = i >> 1;
        const uint32_t b0 = row[8 * j + 2 * t], b1 = row[8 * j + 2 * t + 1];
        const uint32_t b2 = row[8 * (j + 1) + 2 * t], b3 = row[8 * (j + 1) + 2 * t + 1];
        reinterpret_cast<uint32_t *>(dst + r * (size_t)d)[p >> 2] = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
}

hipError_t launch_rerank_permute(hipStream_t s, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t count, int d)
{
    if (count == 0)
        return hipSuccess;
    const size_t words = count * (size_t)(d / 4);
    const unsigned grid = (unsigned)std::min<size_t>((words + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(rerank_permute_kernel<false>, dim3(grid), dim3(256), 0, s, src, src_stride, dst, count, d, nullptr);
    return hipGetLastError();
}

hipError_t launch_rerank_permute_rows(hipStream_t s, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t count, int d,
                                      const int32_t *row_src)
{
    if (count == 0)
        return hipSuccess;
    const size_t words = count * (size_t)(d / 4);
    const unsigned grid = (unsigned)std::min<size_t>((words + 255) / 256, 256 * 64);
    hipLaunchKernelGGL(rerank_permute_kernel<true>, dim3(grid), dim3(256), 0, s, src, src_stride, dst, count, d, row_src);
    return hipGetLastError();
}

// ---- the re-rank -----------------------------------------------------------------------------------------------------
// One lane's contribution to a row: its NW dwords (NW = d/16; template form for the common d, runtime otherwise).
template <int NW>
__device__ __forceinline__ void rr_load(const uint8_t *p, uint32_t (&w)[NW])
{
    if constexpr (NW % 4 == 0) {
#pragma unroll
        for (int i = 0; i < NW / 4; i++) {
            const uint4 v = reinterpret_cast<const uint4 *>(p)[i];
            w[4 * i] = v.x;
            w[4 * i + 1] = v.y;
            w[4 * i + 2] = v.z;
            w[4 * i + 3] = v.w;
        }
    } else if constexpr (NW % 2 == 0) {
#pragma unroll
        for (int i = 0; i < NW / 2; i++) {
            const uint2 v = reinterpret_cast<const uint2 *>(p)[i];
            w[2 * i] = v.x;
            w[2 * i + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int i = 0; i < NW; i++)
            w[i] = reinterpret_cast<const uint32_t *>(p)[i];
    }
}

// acc over one dword = stored bytes 4i..4i+3 of the slice = (dim 8(2i)+2t, +1), (dim 8(2i+1)+2t, +1): block order kept
__device__ __forceinline__ void rr_acc_word(uint32_t w, const float *qs, float &alo, float &ahi)
{
    const float4 q = *reinterpret_cast<const float4 *>(qs);
    float t0 = __fsub_rn(q.x, (float)(w & 0xff)), t1 = __fsub_rn(q.y, (float)((w >> 8) & 0xff));
    alo = __fadd_rn(alo, __fmul_rn(t0, t0));
    ahi = __fadd_rn(ahi, __fmul_rn(t1, t1));
    t0 = __fsub_rn(q.z, (float)((w >> 16) & 0xff));
    t1 = __fsub_rn(q.w, (float)(w >> 24));
    alo = __fadd_rn(alo, __fmul_rn(t0, t0));
    ahi = __fadd_rn(ahi, __fmul_rn(t1, t1));
}

__device__ __forceinline__ float rr_quad_total(float alo, float ahi)
{
    float r = __fadd_rn(quad_bcast<0>(alo), quad_bcast<0>(ahi));
    r = __fadd_rn(r, quad_bcast<1>(alo));
    r = __fadd_rn(r, quad_bcast<1>(ahi));
    r = __fadd_rn(r, quad_bcast<2>(alo));
    r = __fadd_rn(r, quad_bcast<2>(ahi));
    r = __fadd_rn(r, quad_bcast<3>(alo));
    r = __fadd_rn(r, quad_bcast<3>(ahi));
    return r;
}

// the keys' LDS, rounded up so that the query slices behind it are 16-byte aligned
__host__ __device__ inline size_t rr_keys_bytes(int P) { return ((size_t)P * 8 + 15) & ~(size_t)15; }

// NW > 0: compile-time d = 16 * NW, R rows per quad in flight.  NW == 0: any d (runtime loop, one row at a time).
template <int NW, int R>
__global__ __launch_bounds__(RR_THREADS_MAX) void rerank_kernel(const uint8_t *__restrict__ base, uint64_t n, int d_rt,
                                                                const float *__restrict__ queries,
                                                                const long long *__restrict__ cand, int kc, int k, int P,
                                                                float *__restrict__ out_dist, long long *__restrict__ out_lab)
{
    extern __shared__ __align__(16) unsigned char rr_lds[];
    const int d = NW > 0 ? 16 * NW : d_rt;
    const int S = d >> 2;  // bytes (= floats of the permuted query) per lane slice
    const int QS = S + 4;  // LDS stride of a slice: lanes t and t+2 of a quad land on different banks
    unsigned long long *keys = reinterpret_cast<unsigned long long *>(rr_lds);
    float *qp = reinterpret_cast<float *>(rr_lds + rr_keys_bytes(P));

    const size_t q = blockIdx.x;
    const int tid = threadIdx.x, nthr = blockDim.x;
    const float *xq = queries + q * (size_t)d;
    for (int p = tid; p < d; p += nthr) { // permuted query: slot t, element i = dim 8(i/2) + 2t + (i%2)
        const int t = p / S, i = p - t * S;
        qp[t * QS + i] = xq[8 * (i >> 1) + 2 * t + (i & 1)];
    }
    for (int i = kc + tid; i < P; i += nthr)
        keys[i] = RR_EMPTY;
    __syncthreads();

    const int quad = tid >> 2, t = tid & 3, nquads = nthr >> 2;
    const float *qs = qp + t * QS;
    const long long *qc = cand + q * (size_t)kc;
    // every lane runs the same trip count (the quad sums are DPP across the quad; all four lanes agree on a row anyway)
    for (int r0 = 0; r0 < kc; r0 += nquads * R) {
        if constexpr (NW > 0) {
            uint32_t w[R][NW];
            bool ok[R];
            long long lab[R];
#pragma unroll
            for (int u = 0; u < R; u++) {
                const int i = r0 + u * nquads + quad;
                lab[u] = i < kc ? qc[i] : -1;
                ok[u] = lab[u] >= 0 && (unsigned long long)lab[u] < n;
                if (ok[u])
                    rr_load<NW>(base + (size_t)lab[u] * d + t * S, w[u]);
                else
#pragma unroll
                    for (int x = 0; x < NW; x++)
                        w[u][x] = 0;
            }
#pragma unroll
            for (int u = 0; u < R; u++) {
                float alo = 0.f, ahi = 0.f;
#pragma unroll
                for (int x = 0; x < NW; x++)
                    rr_acc_word(w[u][x], qs + 4 * x, alo, ahi);
                const float dist = rr_quad_total(alo, ahi);
                const int i = r0 + u * nquads + quad;
                if (t == 0 && i < kc)
                    keys[i] = ok[u] ? ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned long long)lab[u]
                                    : RR_EMPTY;
            }
        } else {
            const int i = r0 + quad;
            const long long lab = i < kc ? qc[i] : -1;
            const bool ok = lab >= 0 && (unsigned long long)lab < n;
            const uint32_t *row = reinterpret_cast<const uint32_t *>(base + (size_t)(ok ? lab : 0) * d + t * S);
            float alo = 0.f, ahi = 0.f;
            for (int x = 0; x < (S >> 2); x++)
                rr_acc_word(ok ? row[x] : 0u, qs + 4 * x, alo, ahi);
            const float dist = rr_quad_total(alo, ahi);
            if (t == 0 && i < kc)
                keys[i] = ok ? ((unsigned long long)__float_as_uint(dist) << 32) | (unsigned long long)lab : RR_EMPTY;
        }
    }
    __syncthreads();

    // bitonic sort of the P keys, ascending
    for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
            for (int j = tid; j < (P >> 1); j += nthr) {
                const int a = 2 * j - (j & (stride - 1)), b = a + stride;
                const unsigned long long ka = keys[a], kb = keys[b];
                const bool up = (a & size) == 0;
                if ((ka > kb) == up) {
                    keys[a] = kb;
                    keys[b] = ka;
                }
            }
            __syncthreads();
        }
    }

    for (int i = tid; i < k; i += nthr) {
        const unsigned long long key = keys[i];
        const bool e = key == RR_EMPTY;
        out_dist[q * (size_t)k + i] = e ? FLT_MAX : __uint_as_float((uint32_t)(key >> 32));
        out_lab[q * (size_t)k + i] = e ? -1ll : (long long)(uint32_t)key;
    }
}

size_t rerank_lds_bytes(int kc, int d)
{
    int P = 1;
    while (P < kc)
        P <<= 1;
    return rr_keys_bytes(P) + (size_t)4 * (d / 4 + 4) * sizeof(float);
}

hipError_t launch_rerank(hipStream_t s, const uint8_t *base, uint64_t n, int d, const float *queries,
                         const int64_t *cand, size_t nq, int kc, int k, float *dist, int64_t *labels)
{
    if (nq == 0)
        return hipSuccess;
    int P = 1;
    while (P < kc)
        P <<= 1;
    const size_t lds = rerank_lds_bytes(kc, d);
    int thr = ((kc * 4 + 63) / 64) * 64;
    thr = thr < 64 ? 64 : thr > RR_THREADS_MAX ? RR_THREADS_MAX : thr;
    const long long *c = reinterpret_cast<const long long *>(cand);
    long long *l = reinterpret_cast<long long *>(labels);
    const size_t kMaxGrid = (size_t)1 << 30;
    for (size_t q0 = 0; q0 < nq; q0 += kMaxGrid) {
        const size_t m = std::min(kMaxGrid, nq - q0);
        const float *xq = queries + q0 * (size_t)d;
        const long long *cq = c + q0 * (size_t)kc;
        float *od = dist + q0 * (size_t)k;
        long long *ol = l + q0 * (size_t)k;
#define RR_LAUNCH(NW, R)                                                                                                 \
    hipLaunchKernelGGL((rerank_kernel<NW, R>), dim3((unsigned)m), dim3(thr), lds, s, base, (unsigned long long)n, d, xq, \
                       cq, kc, k, P, od, ol)
        switch (d) {
        case 128: RR_LAUNCH(8, 2); break;
        case 96: RR_LAUNCH(6, 2); break;
        case 64: RR_LAUNCH(4, 4); break;
        case 256: RR_LAUNCH(16, 1); break;
        case 512: RR_LAUNCH(32, 1); break;
        default: RR_LAUNCH(0, 1); break;
        }
#undef RR_LAUNCH
        hipError_t e = hipGetLastError();
        if (e != hipSuccess)
            return e;
    }
    return hipSuccess;
}

} // namespace ivfhnsw_gpu_impl
