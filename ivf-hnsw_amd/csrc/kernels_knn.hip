// Exact k-nearest-neighbour tables by brute force on the matrix cores (the open half of row f4).
//
// What it stands for in the reference: every construction step that asks "which stored vectors are nearest to this one"
// -- hnswlib's addPoint finds a new node's link candidates with an efConstruction-wide search of the graph built so far
// (hnswlib/hnswalg.cpp:112-225), Grouping's add_group asks the graph for the nsubc + 1 nearest centroids of a centroid
// (IndexIVF_HNSW_Grouping.cpp:47-62), and the drivers score Recall@1 against ground-truth files that are exact brute
// force (tests/test_ivfhnsw_sift1b.cpp:173-215).  All three are approximations of, or ARE, the exact table this kernel
// computes; the bench and the tests use it to build million-node neighbour graphs, Grouping neighbour tables and ground
// truth without leaving the library.
//
// Arithmetic (the contract the oracle restates, orc_knn):
//     norm(v)    = fmaf chain over k = 0..d-1 of v[k] * v[k], starting from 0
//     dot(q, x)  = fmaf chain over k = 0..d-1 of q[k] * x[k]      -- v_mfma_f32_32x32x2_f32 is exactly that chain
//     dist(q, x) = (norm(q) + norm(x)) - 2 * dot(q, x)            -- two rounded operations, 2 * dot is exact
//     result     = the k smallest (dist, id) pairs, ascending
// This IS a dense contraction (nq x d times d x nx), so it belongs on MFMA; it is not the reference's search-time
// distance (the walk keeps hnswalg.cpp:326-357's order, kernels_hnsw.hip).
//
// Shape: a 256-thread workgroup owns 128 query rows, wave w the 32-row strip [32w, 32w + 32).  The strip (operand A:
// lane l feeds q[row l % 32][k = 2j + l / 32]) stays in d/2 registers for the whole sweep; the workgroup streams x in
// tiles of 32 columns through LDS, stored k-major ([k][32 columns]: the staging writes and the operand-B reads of a
// half-wave both touch 32 consecutive words, no bank conflicts); the next tile's global loads are in flight in
// registers behind the current tile's d/2 MFMAs (one LDS tile, so that with k <= 16 two workgroups fit a CU and fill
// each other's barriers).  Selection is sweep_steps.h's (row_append, rows_compact, rows_write_out), shared with
// kernels_exact.hip; here the key is (orderable distance, id).  Few query rows (ground truth for 10 k queries): the
// columns are split over blockIdx.y and the partial tables merged by knn_merge_kernel (sweep_merge).
#include "sweep_steps.h"

#include <float.h>

namespace ivfhnsw_gpu_impl {

namespace {

typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void knn_norms_kernel(const float *__restrict__ x, float *__restrict__ out, size_t n, int d,
                                                        int ld)
{
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n)
        return;
    const float *r = x + i * (size_t)ld;
    float acc = 0.f;
    for (int k = 0; k < d; k++)
        acc = __fmaf_rn(r[k], r[k], acc);
    out[i] = acc;
}

// D2 = padded d / 2 (rows are read as `d` floats, the rest of the chain multiplies zeros: fmaf(0, 0, acc) = acc)
// CAP = entries of a row's candidate buffer; a row is compacted when it holds more than CAP - 32
template <int D2, int CAP>
__global__ __launch_bounds__(256, 2) void knn_mfma_kernel(const float *__restrict__ Q, const float *__restrict__ X,
                                                          const float *__restrict__ qn, const float *__restrict__ xn,
                                                          int nq, size_t nx, int d, int k, int mode,
                                                          size_t cols_per_split,
                                                          unsigned long long *__restrict__ out_keys)
{
    constexpr int DP = 2 * D2;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float *s_x = reinterpret_cast<float *>(smem);                                       // [DP][32]
    float *s_xn = s_x + DP * 32;                                                        // [32]
    unsigned long long *s_buf = reinterpret_cast<unsigned long long *>(s_xn + 32);      // [4][32][CAP]
    uint32_t *s_cnt = reinterpret_cast<uint32_t *>(s_buf + 4 * 32 * CAP);               // [4][32]
    float *s_thr = reinterpret_cast<float *>(s_cnt + 128);                              // [4][32]

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int m = lane & 31, kk = lane >> 5;
    const int r0 = blockIdx.x * 128 + wave * 32;
    const size_t c_begin = (size_t)blockIdx.y * cols_per_split;
    size_t c_end = c_begin + cols_per_split < nx ? c_begin + cols_per_split : nx;
    // mode 2 (only EARLIER rows are candidates: the neighbour table of an incremental construction, row i against
    // rows 0..i-1): columns at and beyond the block's last row are never candidates
    if (mode == 2 && c_end > (size_t)(blockIdx.x + 1) * 128)
        c_end = (size_t)(blockIdx.x + 1) * 128;
    unsigned long long *buf = s_buf + (size_t)wave * 32 * CAP;
    uint32_t *cnt = s_cnt + wave * 32;
    float *thr_s = s_thr + wave * 32;

    // operand A: the wave's 32 query rows, d/2 registers per lane
    float a[D2];
    {
        const int row = min(r0 + m, nq - 1);
        const float *qr = Q + (size_t)row * d;
#pragma unroll
        for (int j = 0; j < D2; j++) {
            const int kx = 2 * j + kk;
            a[j] = kx < d ? qr[kx] : 0.f;
        }
    }
    // the 16 rows whose dot products this lane holds (C/D layout of the 32x32 MFMA)
    float qn_r[16], thr[16];
#pragma unroll
    for (int r = 0; r < 16; r++) {
        qn_r[r] = qn[min(r0 + mfma32_row(r, kk), nq - 1)];
        thr[r] = FLT_MAX;
    }
    if (lane < 32) {
        cnt[lane] = 0;
        thr_s[lane] = FLT_MAX;
    }

    // staging: thread -> (column tid % 32, 16 floats starting at (tid / 32) * 16) of the tile
    const int st_col = tid & 31, st_k0 = (tid >> 5) * 16;
    float4 pre[4];
    float pre_n = 0.f;
    auto fetch = [&](size_t c0) {
        const size_t c = c0 + st_col;
        const bool ok = c < c_end;
        const float *xr = X + (ok ? c : 0) * (size_t)d;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int kx = st_k0 + 4 * i;
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (ok && kx + 3 < d)
                v = *reinterpret_cast<const float4 *>(xr + kx);
            else if (ok && kx < d) {
                v.x = xr[kx];
                v.y = kx + 1 < d ? xr[kx + 1] : 0.f;
                v.z = kx + 2 < d ? xr[kx + 2] : 0.f;
            }
            pre[i] = v;
        }
        if (tid < 32)
            pre_n = ok ? xn[c] : 0.f;
    };
    auto stash = [&]() {
        float *dst = s_x;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int kx = st_k0 + 4 * i;
            if (kx < DP) {
                dst[(kx + 0) * 32 + st_col] = pre[i].x;
                dst[(kx + 1) * 32 + st_col] = pre[i].y;
                dst[(kx + 2) * 32 + st_col] = pre[i].z;
                dst[(kx + 3) * 32 + st_col] = pre[i].w;
            }
        }
        if (tid < 32)
            s_xn[tid] = pre_n;
    };

    fetch(c_begin);
    for (size_t c0 = c_begin; c0 < c_end; c0 += 32) {
        __syncthreads(); // the previous tile has been consumed by every wave
        stash();
        __syncthreads();
        if (c0 + 32 < c_end)
            fetch(c0 + 32); // in flight behind this tile's MFMAs
        const float *xt = s_x;
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int j = 0; j < D2; j++)
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[j], xt[(2 * j + kk) * 32 + m], acc, 0, 0, 0);
        const float xnc = s_xn[m];
        const size_t col = c0 + m;
        const bool col_ok = col < c_end;
        bool any_new = false;
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const float dist = __fsub_rn(__fadd_rn(qn_r[r], xnc), __fmul_rn(2.0f, acc[r]));
            const int row = mfma32_row(r, kk);
            const bool pass = col_ok && dist < thr[r] && (mode == 0 || (mode == 1 ? (long long)col != (long long)(r0 + row)
                                                                                   : (long long)col < (long long)(r0 + row)));
            const unsigned long long mask = __ballot(pass);
            if (mask) { // wave-uniform: rare once the thresholds have settled
                row_append<CAP>(buf, cnt, row, pass, mask, dist, (uint32_t)col, m, kk);
                any_new = true;
            }
        }
        if (any_new) {
            rows_compact<CAP>(buf, cnt, thr_s, k, lane);
#pragma unroll
            for (int r = 0; r < 16; r++)
                thr[r] = thr_s[mfma32_row(r, kk)];
        }
    }

    // out: [split][nq][k] keys
    rows_write_out<CAP>(buf, cnt, k, lane, nq - r0, out_keys, (size_t)blockIdx.y * nq + r0);
}

__global__ __launch_bounds__(64) void knn_merge_kernel(const unsigned long long *__restrict__ part, int nsplit, int nq,
                                                       int k, uint32_t *__restrict__ ids, float *__restrict__ dists)
{
    sweep_merge(
        part, nsplit, nq, k,
        [&](size_t o, unsigned long long key) {
            ids[o] = (uint32_t)key;
            dists[o] = orderable_f32((uint32_t)(key >> 32));
        },
        [&](size_t o) {
            ids[o] = 0xffffffffu;
            dists[o] = FLT_MAX;
        });
}

template <int D2, int CAP>
hipError_t launch_knn_t(hipStream_t s, const float *Q, const float *X, const float *qn, const float *xn, int nq, size_t nx,
                        int d, int k, int mode, int nsplit, size_t cols_per_split, unsigned long long *part)
{
    const size_t shm = (size_t)(2 * D2 * 32 + 32) * sizeof(float) + (size_t)4 * 32 * CAP * sizeof(unsigned long long) +
                       128 * sizeof(uint32_t) + 128 * sizeof(float);
    constexpr auto kern = knn_mfma_kernel<D2, CAP>;
    if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
        return e;
    hipLaunchKernelGGL(kern, dim3((unsigned)((nq + 127) / 128), (unsigned)nsplit), dim3(256), shm, s, Q, X, qn, xn, nq, nx, d,
                       k, mode, cols_per_split, part);
    return hipGetLastError();
}

} // namespace

hipError_t launch_knn_norms(hipStream_t s, const float *x, float *out, size_t n, int d)
{
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(knn_norms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, x, out, n, d, d);
    return hipGetLastError();
}

// part: [nsplit][nq][k] u64 workspace
hipError_t launch_knn(hipStream_t s, const float *Q, const float *X, const float *qn, const float *xn, size_t nq, size_t nx,
                      int d, int k, int mode, int nsplit, unsigned long long *part, uint32_t *ids, float *dists)
{
    if (nq == 0 || k == 0)
        return hipSuccess;
    if (d < 4 || d > 128 || (d & 3) || k > 80 || nq > 0x7fffffffull || nx > 0xffffffffull || nsplit < 1 || mode < 0 || mode > 2)
        return hipErrorInvalidValue;
    const size_t cps = sweep_cols_per_split(nx, nsplit);
    hipError_t e;
    const int d2 = (d + 1) / 2;
#define IVFHNSW_KNN(D2)                                                                                                \
    (k <= 16   ? launch_knn_t<D2, 48>(s, Q, X, qn, xn, (int)nq, nx, d, k, mode, nsplit, cps, part)              \
     : k <= 32 ? launch_knn_t<D2, 64>(s, Q, X, qn, xn, (int)nq, nx, d, k, mode, nsplit, cps, part)              \
               : launch_knn_t<D2, 112>(s, Q, X, qn, xn, (int)nq, nx, d, k, mode, nsplit, cps, part))
    if (d2 <= 16)
        e = IVFHNSW_KNN(16);
    else if (d2 <= 32)
        e = IVFHNSW_KNN(32);
    else if (d2 <= 48)
        e = IVFHNSW_KNN(48);
    else
        e = IVFHNSW_KNN(64);
#undef IVFHNSW_KNN
    if (e != hipSuccess)
        return e;
    hipLaunchKernelGGL(knn_merge_kernel, dim3((unsigned)nq), dim3(64), 0, s, part, nsplit, (int)nq, k, ids, dists);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
