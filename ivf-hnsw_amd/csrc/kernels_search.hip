// gfx950 kernels of the IVFADC search path: OPQ rotation, PQ inner-product table, IVF scan plan,
// ADC list scan, label resolution, synthetic corpus fill.
//
// Float contract (see DESIGN.md "Numerics"): every arithmetic step is an explicit round-to-nearest
// intrinsic in the order the reference's source evaluates it; this file is built with
// -ffp-contract=off so nothing else gets fused either.
#include "plan_steps.h"
#include "scan_steps.h"
#include "sweep_steps.h"

#include <float.h>
#include <stdlib.h>
#include <algorithm>

namespace ivfhnsw_gpu_impl {

// ---------------------------------------------------------------------------------------------
// OPQ rotation: y[q][i] = sum_k A[i][k] x[q][k] as a k-ordered fmaf chain (reference call site
// IndexIVF_HNSW.cpp:240; faiss hands this to sgemm, whose order is unspecified).
// One block per query, one thread per output dim; At is A transposed so reads coalesce.
// ---------------------------------------------------------------------------------------------
__global__ void opq_kernel(const float *__restrict__ At, const float *__restrict__ x, float *__restrict__ y, int nq,
                           int d)
{
    extern __shared__ float s_x[];
    const int q = blockIdx.x;
    for (int i = threadIdx.x; i < d; i += blockDim.x)
        s_x[i] = x[(size_t)q * d + i];
    __syncthreads();
    for (int i = threadIdx.x; i < d; i += blockDim.x) {
        float acc = 0.0f;
        for (int k = 0; k < d; k++)
            acc = __fmaf_rn(At[(size_t)k * d + i], s_x[k], acc);
        y[(size_t)q * d + i] = acc;
    }
}

// Batched form on the matrix cores -- the one true dense contraction on the path (nq x d times d x d).
// v_mfma_f32_32x32x2_f32 computes D = A*B + C as a k-ordered fmaf chain per element, one rounding per step
// (MI355X guide: "bit-for-bit a k-ordered f32 fmaf chain"), which is exactly the order opq_kernel and the
// oracle use, so the result is bit-identical to the scalar form.
// One 256-thread workgroup = 32 queries x up to 128 output dims: wave w owns the 32x32 tile of output dims
// [32w, 32w+32).  MFMA operand A = x (row = query, k), operand B = At (k, output dim): lane l feeds
// x[q0 + l%32][k0 + l/32] and At[k0 + l/32][i0 + l%32]; the query tile sits in LDS with a padded row so the
// 32 lanes of a read hit 32 banks.
typedef float f32x16 __attribute__((ext_vector_type(16)));

__global__ __launch_bounds__(256) void opq_mfma_kernel(const float *__restrict__ At, const float *__restrict__ x,
                                                       float *__restrict__ y, int nq, int d)
{
    extern __shared__ float s_xt[]; // [32][d + 1]
    const int q0 = blockIdx.x * 32;
    const int ld = d + 1;
    for (int i = threadIdx.x; i < 32 * d; i += 256) {
        const int r = i / d, c = i - r * d;
        const int q = min(q0 + r, nq - 1); // rows past the batch replicate the last query; never stored
        s_xt[r * ld + c] = x[(size_t)q * d + c];
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int m = lane & 31, kk = lane >> 5;
    for (int i0 = (blockIdx.y * 4 + wave) * 32; i0 < d; i0 += gridDim.y * 128) {
        f32x16 acc = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
        for (int k0 = 0; k0 < d; k0 += 2) {
            const float a = s_xt[m * ld + k0 + kk];
            const float b = At[(size_t)(k0 + kk) * d + i0 + m];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
#pragma unroll
        for (int r = 0; r < 16; r++) {
            const int row = mfma32_row(r, kk);
            if (q0 + row < nq)
                y[(size_t)(q0 + row) * d + i0 + m] = acc[r];
        }
    }
}

hipError_t launch_opq(hipStream_t s, const float *At, const float *x, float *y, int nq, int d)
{
    if (nq == 0)
        return hipSuccess;
    if (d % 32 == 0 && d <= 2048) {
        const size_t shm = (size_t)32 * (d + 1) * sizeof(float);
        hipLaunchKernelGGL(opq_mfma_kernel, dim3((nq + 31) / 32, (d + 127) / 128), dim3(256), shm, s, At, x, y, nq, d);
        return hipGetLastError();
    }
    int threads = d < 256 ? ((d + 63) / 64) * 64 : 256;
    hipLaunchKernelGGL(opq_kernel, dim3(nq), dim3(threads), d * sizeof(float), s, At, x, y, nq, d);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// PQ inner-product table (IndexIVF_HNSW.cpp:262): tab[q][m][c] = <x_m, centroid[m][c]>.
// Order inside one product = faiss's SSE fvec_inner_product: 4 partial sums over blocks of 4,
// zero-padded tail, then (s0+s1)+(s2+s3).
// One block = LUT_QB queries x 256 code words: thread c keeps centroid[m][c][:] in registers and
// reuses it for the block's queries, so the 128 KB codebook is read once per LUT_QB queries.
// ---------------------------------------------------------------------------------------------
constexpr int LUT_QB = 4;

template <int DSUB>
__device__ __forceinline__ void lut_body(int bid, float *s_q, const float *__restrict__ xq, const float *__restrict__ cb,
                                         float *__restrict__ luts, int nq, int d, int M, int dsub_rt,
                                         const PlanHdr *__restrict__ hdr)
{
    const int dsub = DSUB > 0 ? DSUB : dsub_rt;
    const int q0 = bid * LUT_QB;
    const int nqb = min(LUT_QB, nq - q0);
    // a shard scores nothing for a query none of whose scanned lists it owns (16 % of the queries at 8 shards):
    // no table needed
    bool need[LUT_QB];
    bool any = false;
#pragma unroll
    for (int qi = 0; qi < LUT_QB; qi++) {
        need[qi] = qi < nqb && (!hdr || hdr[q0 + qi].total != 0);
        any |= need[qi];
    }
    if (!any)
        return;
    for (int i = threadIdx.x; i < nqb * d; i += 256)
        s_q[i] = xq[(size_t)q0 * d + i];
    __syncthreads();
    const int c = threadIdx.x;
    constexpr int RMAX = DSUB > 0 ? DSUB : 64;
    float row[RMAX];
    for (int m = 0; m < M; m++) {
        const float *src = cb + ((size_t)m * 256 + c) * dsub;
        if constexpr (DSUB > 0 && DSUB % 4 == 0) {
#pragma unroll
            for (int i = 0; i < DSUB; i += 4) {
                float4 v = *reinterpret_cast<const float4 *>(src + i);
                row[i] = v.x, row[i + 1] = v.y, row[i + 2] = v.z, row[i + 3] = v.w;
            }
        } else {
            for (int i = 0; i < dsub; i++)
                row[i] = src[i];
        }
#pragma unroll
        for (int qi = 0; qi < LUT_QB; qi++) {
            if (!need[qi])
                continue;
            float r = ip_sse_order<DSUB>(s_q + qi * d + m * dsub, row, dsub);
            luts[((size_t)(q0 + qi) * M + m) * 256 + c] = r;
        }
    }
}

template <int DSUB>
__global__ __launch_bounds__(256) void lut_kernel(const float *__restrict__ xq, const float *__restrict__ cb,
                                                  float *__restrict__ luts, int nq, int d, int M, int dsub_rt,
                                                  const PlanHdr *__restrict__ hdr)
{
    extern __shared__ float s_q[]; // [LUT_QB][d]
    lut_body<DSUB>((int)blockIdx.x, s_q, xq, cb, luts, nq, d, M, dsub_rt, hdr);
}

hipError_t launch_lut(hipStream_t s, const IvfTables &t, const float *xq, float *luts, int nq, const PlanHdr *hdr)
{
    if (nq == 0)
        return hipSuccess;
    dim3 grid((nq + LUT_QB - 1) / LUT_QB), block(256);
    size_t shm = (size_t)LUT_QB * t.d * sizeof(float);
    switch (t.dsub) {
    case 4: hipLaunchKernelGGL(lut_kernel<4>, grid, block, shm, s, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, hdr); break;
    case 6: hipLaunchKernelGGL(lut_kernel<6>, grid, block, shm, s, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, hdr); break;
    case 8: hipLaunchKernelGGL(lut_kernel<8>, grid, block, shm, s, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, hdr); break;
    case 12: hipLaunchKernelGGL(lut_kernel<12>, grid, block, shm, s, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, hdr); break;
    case 16: hipLaunchKernelGGL(lut_kernel<16>, grid, block, shm, s, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, hdr); break;
    default:
        if (t.dsub > 64)
            return hipErrorInvalidValue;
        hipLaunchKernelGGL(lut_kernel<0>, grid, block, shm, s, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, hdr);
    }
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// IVF scan plan (IndexIVF_HNSW.cpp:267-292): probes nearest first, empty lists skipped, stop after
// the list that makes ncode >= max_codes.  Depends only on coarse results and list sizes, never on
// codes, so it is computed up front and the scan itself is order-free.
// ---------------------------------------------------------------------------------------------
// One wavefront per query, lanes over the probes (chunks of 64, ivf_plan_chunk in plan_steps.h): list sizes in parallel,
// the max_codes prefix rule by a wave scan -- list i is scored iff fewer than max_codes codes precede it in probe order.
__device__ __forceinline__ void plan_ivf_body(int bid, const IvfTables &t, const uint32_t *__restrict__ cid,
                                              const float *__restrict__ cd, int nq, int nprobe,
                                              unsigned long long max_codes, Seg *__restrict__ segs,
                                              uint32_t *__restrict__ lpos, PlanHdr *__restrict__ hdr, int max_seg,
                                              unsigned long long *__restrict__ keys, int k)
{
    const int q = bid * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (q >= nq)
        return;
    for (int j = lane; j < k; j += 64)
        keys[(size_t)q * k + j] = kKeyInit;
    PlanCursor cur;
    for (int base = 0; base < nprobe && plan_budget_open(cur.ncode, max_codes); base += 64)
        ivf_plan_chunk(cur, t, cid + (size_t)q * nprobe, cd + (size_t)q * nprobe, base, nprobe, max_codes,
                       segs + (size_t)q * max_seg, lpos + (size_t)q * max_seg, lane);
    if (lane == 0)
        store_plan_hdr(&hdr[q], cur.ns, cur.nl);
}

__global__ __launch_bounds__(256) void plan_ivf_kernel(IvfTables t, const uint32_t *__restrict__ cid,
                                                       const float *__restrict__ cd, int nq, int nprobe,
                                                       unsigned long long max_codes, Seg *__restrict__ segs,
                                                       uint32_t *__restrict__ lpos, PlanHdr *__restrict__ hdr,
                                                       int max_seg, unsigned long long *__restrict__ keys, int k)
{
    plan_ivf_body((int)blockIdx.x, t, cid, cd, nq, nprobe, max_codes, segs, lpos, hdr, max_seg, keys, k);
}

// Plan and tables of one batch in ONE launch (one GPU, IVFADC): they are independent of each other -- the plan needs the
// coarse results, the tables the queries -- and the plan's 15 us of dependent list-size reads hide behind the tables'
// 50 us of writes.  (On a list shard the table kernel skips queries the shard has nothing for, which it learns from the
// plan: there the two stay separate launches.)  Blocks [0, plan_blocks) plan four queries each, the rest build tables.
template <int DSUB>
__global__ __launch_bounds__(256) void plan_lut_kernel(IvfTables t, const uint32_t *__restrict__ cid,
                                                       const float *__restrict__ cd, int nq, int nprobe,
                                                       unsigned long long max_codes, Seg *__restrict__ segs,
                                                       uint32_t *__restrict__ lpos, PlanHdr *__restrict__ hdr,
                                                       int max_seg, unsigned long long *__restrict__ keys, int k,
                                                       int plan_blocks, const float *__restrict__ xq,
                                                       float *__restrict__ luts)
{
    extern __shared__ float s_q[]; // [LUT_QB][d]
    if ((int)blockIdx.x < plan_blocks)
        plan_ivf_body((int)blockIdx.x, t, cid, cd, nq, nprobe, max_codes, segs, lpos, hdr, max_seg, keys, k);
    else
        lut_body<DSUB>((int)blockIdx.x - plan_blocks, s_q, xq, t.pq_centroids, luts, nq, t.d, t.M, t.dsub, nullptr);
}

hipError_t launch_plan_lut(hipStream_t s, const IvfTables &t, const float *xq, const uint32_t *coarse_ids,
                           const float *coarse_dists, int nprobe, uint64_t max_codes, const PlanView &p, uint64_t *keys,
                           int k, float *luts)
{
    const auto [segs, lpos, hdr, max_seg, nq] = p;
    if (nq == 0)
        return hipSuccess;
    const int plan_blocks = (nq + 3) / 4, lut_blocks = (nq + LUT_QB - 1) / LUT_QB;
    const dim3 grid(plan_blocks + lut_blocks), block(256);
    const size_t shm = (size_t)LUT_QB * t.d * sizeof(float);
    auto *k64 = reinterpret_cast<unsigned long long *>(keys);
#define IVFHNSW_PLAN_LUT(DS)                                                                                          \
    hipLaunchKernelGGL(plan_lut_kernel<DS>, grid, block, shm, s, t, coarse_ids, coarse_dists, nq, nprobe,             \
                       (unsigned long long)max_codes, segs, lpos, hdr, max_seg, k64, k, plan_blocks, xq, luts)
    switch (t.dsub) {
    case 4: IVFHNSW_PLAN_LUT(4); break;
    case 6: IVFHNSW_PLAN_LUT(6); break;
    case 8: IVFHNSW_PLAN_LUT(8); break;
    case 12: IVFHNSW_PLAN_LUT(12); break;
    case 16: IVFHNSW_PLAN_LUT(16); break;
    default: return hipErrorInvalidValue; // the caller keeps the two launches for other shapes
    }
#undef IVFHNSW_PLAN_LUT
    return hipGetLastError();
}

hipError_t launch_plan_ivf(hipStream_t s, const IvfTables &t, const uint32_t *coarse_ids, const float *coarse_dists,
                           int nprobe, uint64_t max_codes, const PlanView &p, uint64_t *keys, int k)
{
    const auto [segs, lpos, hdr, max_seg, nq] = p;
    if (nq == 0)
        return hipSuccess;
    hipLaunchKernelGGL(plan_ivf_kernel, dim3((nq + 3) / 4), dim3(256), 0, s, t, coarse_ids, coarse_dists, nq,
                       nprobe, (unsigned long long)max_codes, segs, lpos, hdr, max_seg,
                       reinterpret_cast<unsigned long long *>(keys), k);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// ADC list scan, k = 1 (IndexIVF_HNSW.cpp:282-289, IndexIVF_HNSW_Grouping.cpp:321-333).
//
// One 256-thread workgroup per (query, split).  The query's 256-entry-per-byte table (CS KB as
// f32) and the 256-entry norm table are staged in LDS; the plan's segments are flattened into one
// virtual array of `total` codes and lane t of iteration it scores position it*256*U + u*256 + t,
// so consecutive lanes read consecutive CS-byte codes (one global_load_dwordx4 per lane for CS=16:
// 1 KiB per wave instruction) and a wave only diverges in its base address at a list boundary.
// Per code: CS LDS gathers summed in m order, dist = (cterm + norm) - 2*sum, packed into a
// (distance, scan position) key; the wave/block minimum is the reference's strict-'<' first-wins top-1.
// Bound: HBM read of CS+1 bytes per code; the CS LDS gathers per code run at about the same rate
// (random bank conflicts), see DESIGN.md.  The steps shared with the other scan kernels: scan_steps.h.  (Replicating the
// table over disjoint LDS banks was built and measured in round 1 -- no gain, DESIGN.md 3.1 -- and removed in round 3.)
// ---------------------------------------------------------------------------------------------

// The winner's label resolved by the scan itself (k = 1, one workgroup per query, results wanted as distance + label):
// select_kernel would re-read the key and the plan for 9 us and a launch.  ids == nullptr: keys only, as before.
struct SelOut {
    const uint32_t *ids;
    float *dist;
    long long *labels;
};

__device__ __forceinline__ void sel_write(const SelOut &so, int q, unsigned long long key, const Seg *sq, uint32_t nseg)
{
    float dv = FLT_MAX;
    long long lb = -1;
    if (key < kKeyInit) {
        dv = orderable_f32((uint32_t)(key >> 32));
        const uint32_t vpos = (uint32_t)key;
        if (nseg != 0) {
            uint32_t a = 0, b = nseg - 1; // last segment with seg.vpos <= vpos (segments are in scan order)
            while (a < b) {
                const uint32_t mid = (a + b + 1) >> 1;
                if (sq[mid].vpos <= vpos)
                    a = mid;
                else
                    b = mid - 1;
            }
            const Seg sg = sq[a];
            if (vpos >= sg.vpos && vpos - sg.vpos < sg.len)
                lb = (long long)so.ids[sg.start + (vpos - sg.vpos)];
        }
    }
    so.dist[q] = dv;
    so.labels[q] = lb;
}

// Mask: empty, the pass mask of a label filter, or filter slots per query (device_common.h filter_mask; DESIGN.md 3.14,
// 3.19): a row whose bit is clear forms no key.
template <int CS, int SEGCAP, int U, int THREADS, class... Mask>
__global__ __launch_bounds__(THREADS) void scan_k1_kernel(const uint8_t *__restrict__ codes,
                                                          const uint8_t *__restrict__ norm_codes,
                                                          const float *__restrict__ luts,
                                                          const float *__restrict__ norm_table,
                                                          const Seg *__restrict__ segs,
                                                          const uint32_t *__restrict__ lpos,
                                                          const PlanHdr *__restrict__ hdr, int max_seg, int nsplit,
                                                          unsigned long long *__restrict__ keys, int cs_rt, SelOut so,
                                                          Mask... fmask_arg)
{
    constexpr bool FILT = sizeof...(Mask) != 0;
    constexpr int FK = filter_kind<Mask...>;
    // CS == 0: run-time code size cs_rt, table in dynamic LDS (code sizes without an instantiation of their own)
    __shared__ __attribute__((aligned(16))) float s_lut_fixed[(CS > 0 ? CS : 1) * 256];
    extern __shared__ __attribute__((aligned(16))) float s_lut_dyn[];
    float *s_lut = CS > 0 ? s_lut_fixed : s_lut_dyn;
    const int csz = CS > 0 ? CS : cs_rt;
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) Seg s_seg[SEGCAP];
    __shared__ uint32_t s_lpos[SEGCAP + 1];
    __shared__ unsigned long long s_red[THREADS / 64];

    const int tid = threadIdx.x;
    const int q = blockIdx.x / nsplit;
    [[maybe_unused]] FilterFill ffill; // filter slots: what a query without a plane reads instead (filter_mask)
    [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(q, ffill, fmask_arg...);
    const int split = blockIdx.x - q * nsplit;
    const PlanHdr h = hdr[q];
    if (h.total == 0) {
        if (so.ids && tid == 0)
            sel_write(so, q, kKeyInit, nullptr, 0);
        return;
    }
    const auto [lo, hi] = scan_slice(h.total, nsplit, split, THREADS);
    if (lo >= hi)
        return;

    stage_table_dma<THREADS>(luts, q, csz, s_lut, tid);
    for (int i = tid; i < 256; i += THREADS)
        s_norm[i] = norm_table[i];

    const Seg *sq = segs + (size_t)q * max_seg;
    const uint32_t *lq = lpos + (size_t)q * max_seg;
    unsigned long long best = kKeyInit;
    // whole lists, at most 64 of them: the next position is in this list or the next one
    using Seek = std::conditional_t<SEGCAP <= 64, SeekLinear, SeekStep2Halves>;

    for (uint32_t cs = 0; cs < h.nseg; cs += SEGCAP) {
        const uint32_t cn = min((uint32_t)SEGCAP, h.nseg - cs);
        const uint32_t ch = plan_chunk_end(lq, cs, cn, h.nseg, h.total);
        __syncthreads(); // previous chunk fully consumed (and LUT staged, first time)
        stage_plan_chunk<THREADS>(sq, lq, cs, cn, ch, s_seg, s_lpos, tid);
        __syncthreads();
        const uint32_t cl = s_lpos[0];
        const uint32_t b0 = max(cl, lo), b1 = min(ch, hi);
        SegCursor c;
        for (uint32_t base = b0; base < b1; base += THREADS * U) {
            CodeRegs<CS> w[U];
            uint32_t nb[U], vp[U];
            [[maybe_unused]] FilterWord<FK> fw[U];
            [[maybe_unused]] uint32_t fb[U];
            float ct[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t p = base + u * THREADS + tid;
                ok[u] = p < b1;
                if (ok[u]) {
                    c.seek<Seek>(p, s_lpos, s_seg, cn);
                    const uint32_t off = p - c.seg_lo;
                    const uint32_t gi = c.seg_start + off;
                    code_fetch<CS>(codes, gi, cs_rt, s_lut, w[u]);
                    load_norm_filter<FK>(norm_codes, fmask, gi, nb[u], fw[u], ffill);
                    if constexpr (FILT)
                        fb[u] = gi & 31u;
                    vp[u] = c.seg_vpos + off;
                    ct[u] = c.seg_ct;
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if constexpr (FILT)
                    ok[u] = ok[u] && filter_pass<FK>(fw[u], fb[u], ffill);
                if (ok[u]) {
                    const float sum = code_sum_lds<CS>(s_lut, w[u]);
                    const float dist = adc_distance(ct[u], s_norm[nb[u]], sum);
                    if (dist < FLT_MAX) { // also rejects NaN, as 'dist < distances[0]' does
                        const unsigned long long key = adc_key(dist, vp[u]);
                        best = key < best ? key : best;
                    }
                }
            }
        }
    }

    best = wave_min_u64(best);
    if ((tid & 63) == 0)
        s_red[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = s_red[0];
#pragma unroll
        for (int i = 1; i < THREADS / 64; i++)
            b = s_red[i] < b ? s_red[i] : b;
        if (nsplit == 1) {
            keys[q] = b;
            if (so.ids)
                sel_write(so, q, b, segs + (size_t)q * max_seg, h.nseg);
        } else if (b < kKeyInit) {
            atomicMin(&keys[q], b);
        }
    }
}

// The scan for SHORT segments (Grouping: a sub-group holds ~16 codes at the reference's nsubc 64).
// scan_k1_kernel deals positions to lanes but searches the segment of every position in the LDS plan; a lane group per
// segment (round 1's scan_k1_short_kernel, tools/experiments/) leaves half the lanes idle -- and the scan is bound by
// LDS instruction issue, so idle lanes cost as much as busy ones.  Here positions are dealt to lanes one code each
// AND the segment comes from a bitmap: one bit per position of the plan chunk, set where a segment starts, plus the
// number of starts before every 64-position word (scan_steps.h BitmapChunk).  Chunks of <= 256 segments and <= 8192
// positions: 23 KB of LDS per workgroup, six workgroups per CU.
template <int CS, int U, class... Mask> // Mask: see scan_k1_kernel
__global__ __launch_bounds__(256) void scan_k1_bitmap_kernel(const uint8_t *__restrict__ codes,
                                                             const uint8_t *__restrict__ norm_codes,
                                                             const float *__restrict__ luts,
                                                             const float *__restrict__ norm_table,
                                                             const Seg *__restrict__ segs,
                                                             const uint32_t *__restrict__ lpos,
                                                             const PlanHdr *__restrict__ hdr, int max_seg, int nsplit,
                                                             unsigned long long *__restrict__ keys, SelOut so,
                                                             Mask... fmask_arg)
{
    constexpr bool FILT = sizeof...(Mask) != 0;
    constexpr int FK = filter_kind<Mask...>;
    __shared__ __attribute__((aligned(16))) float s_lut[CS * 256];
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) Seg s_seg[kBmSegCap];
    __shared__ uint32_t s_lpos[kBmSegCap + 1];
    __shared__ unsigned long long s_mask[kBmSpanWords];
    __shared__ uint32_t s_pref[kBmSpanWords];
    __shared__ uint32_t s_wtot[4];
    __shared__ unsigned long long s_red[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / nsplit;
    [[maybe_unused]] FilterFill ffill; // filter slots: what a query without a plane reads instead (filter_mask)
    [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(q, ffill, fmask_arg...);
    const int split = blockIdx.x - q * nsplit;
    const PlanHdr h = hdr[q];
    if (h.total == 0) {
        if (so.ids && tid == 0)
            sel_write(so, q, kKeyInit, nullptr, 0);
        return;
    }
    const auto [lo, hi] = scan_slice(h.total, nsplit, split, 256);
    if (lo >= hi)
        return;
    stage_table_dma<256>(luts, q, CS, s_lut, tid);
    s_norm[tid] = norm_table[tid];
    const Seg *sq = segs + (size_t)q * max_seg;
    const uint32_t *lq = lpos + (size_t)q * max_seg;
    unsigned long long best = kKeyInit;

    uint32_t cs = first_segment(lq, h.nseg, lo);
    while (cs < h.nseg) {
        const uint32_t cl = lq[cs];
        if (cl >= hi)
            break;
        const BitmapChunk bc = stage_bitmap_chunk<256>(sq, lq, cs, h.nseg, h.total, s_seg, s_lpos, s_mask, s_pref, s_wtot, tid);
        const uint32_t b0 = max(cl, lo), b1 = min(bc.ch, hi);
        if (b0 < b1) {
            for (uint32_t rbase = (b0 - cl) & ~63u; rbase < b1 - cl; rbase += 256 * U) {
                CodeRegs<CS> w[U];
                uint32_t nb[U], vp[U];
                [[maybe_unused]] FilterWord<FK> fw[U];
                [[maybe_unused]] uint32_t fb[U];
                float ct[U];
                bool ok[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t r = rbase + u * 256 + tid;
                    const uint32_t p = cl + r;
                    ok[u] = p >= b0 && p < b1;
                    const uint32_t wi = BitmapChunk::word_of(r);
                    if (wi * 64u < b1 - cl) { // wave-uniform
                        const uint32_t sgi = bc.segment_of(wi, lane);
                        if (ok[u]) {
                            const Seg sg = s_seg[sgi];
                            const uint32_t off = p - s_lpos[sgi];
                            const uint32_t gi = sg.start + off;
                            code_fetch<CS>(codes, gi, CS, s_lut, w[u]);
                            load_norm_filter<FK>(norm_codes, fmask, gi, nb[u], fw[u], ffill);
                            if constexpr (FILT)
                                fb[u] = gi & 31u;
                            vp[u] = sg.vpos + off;
                            ct[u] = sg.cterm;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if constexpr (FILT)
                        ok[u] = ok[u] && filter_pass<FK>(fw[u], fb[u], ffill);
                    if (ok[u]) {
                        const float sum = code_sum<CS>(s_lut, w[u]);
                        const float dist = adc_distance(ct[u], s_norm[nb[u]], sum);
                        if (dist < FLT_MAX) {
                            const unsigned long long key = adc_key(dist, vp[u]);
                            best = key < best ? key : best;
                        }
                    }
                }
            }
        }
        cs += bc.cn;
    }
    best = wave_min_u64(best);
    if (lane == 0)
        s_red[wave] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long m = s_red[0];
#pragma unroll
        for (int i = 1; i < 4; i++)
            m = s_red[i] < m ? s_red[i] : m;
        if (nsplit == 1) {
            keys[q] = m;
            if (so.ids)
                sel_write(so, q, m, segs + (size_t)q * max_seg, h.nseg);
        } else if (m < kKeyInit) {
            atomicMin(&keys[q], m);
        }
    }
}

hipError_t launch_scan_topk(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int k, uint64_t *keys,
                            const ScanOut &out, const ScanFilter &fmask);

hipError_t launch_scan(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int k, int nsplit,
                       uint64_t *keys, int seg_len_hint, const ScanFilter &fmask, const ScanOut &out, bool *did_select,
                       const char **kernel_name)
{
    bool unused_sel;
    const char *unused_name;
    did_select = did_select ? did_select : &unused_sel; // both out-arguments may be null
    kernel_name = kernel_name ? kernel_name : &unused_name;
    *did_select = false;
    *kernel_name = "";
    if (p.nq == 0)
        return hipSuccess;
    if (k != 1) {
        *kernel_name = fmask.name("scan_topk_kernel", "scan_topk_kernel+filter", "scan_topk_kernel+slots", "scan_topk_kernel+tags", "scan_topk_kernel+values", "scan_topk_kernel+tags+values");
        return launch_scan_topk(s, t, luts, p, k, keys, out, fmask);
    }
    // several workgroups per query meet in an atomic: nobody knows the winner
    const bool sel = out.sel_dist && out.sel_labels && nsplit == 1;
    const SelOut so{sel ? t.ids : nullptr, out.sel_dist, reinterpret_cast<long long *>(out.sel_labels)};
    const dim3 grid((unsigned)p.nq * nsplit), block(256);
    auto *k64 = reinterpret_cast<unsigned long long *>(keys);
    return by_code_size<4, 8, 16, 32>(t.M, [&](auto cs) {
        return with_mask(fmask, [&](auto... m) -> hipError_t {
            constexpr int CS = decltype(cs)::value;
            // the position form: a compiled size unrolls by 4 and stages as many segments as the plan's width asks for
            auto position = [&](auto segcap, auto unroll, const SelOut &so_) -> hipError_t {
                constexpr auto kern = scan_k1_kernel<CS, decltype(segcap)::value, decltype(unroll)::value, 256, decltype(m)...>;
                size_t shm;
                if (hipError_t e = scan_table_lds<CS, kern>(t.M, &shm); e != hipSuccess)
                    return e;
                hipLaunchKernelGGL(kern, grid, block, shm, s, t.codes, t.norm_codes, luts, t.norm_table, p.segs, p.lpos, p.hdr,
                                   p.max_seg, nsplit, k64, t.M, so_, m...);
                *did_select = so_.ids != nullptr;
                return hipGetLastError();
            };
            if constexpr (CS == 0) {
                // any other multiple of 4 (IndexIVF_HNSW.cpp:805): the run-time form, table in dynamic LDS, keys only
                *kernel_name = fmask.name("scan_k1_kernel (run-time code size)", "scan_k1_kernel (run-time code size)+filter",
                                          "scan_k1_kernel (run-time code size)+slots", "scan_k1_kernel (run-time code size)+tags", "scan_k1_kernel (run-time code size)+values", "scan_k1_kernel (run-time code size)+tags+values");
                return position(int_c<256>(), int_c<2>(), SelOut{nullptr, nullptr, nullptr});
            } else if (seg_len_hint > 0 && seg_len_hint <= 48) {
                // plans of short segments (Grouping sub-groups, ~16 codes): the bitmap form; whole lists: the position form
                *kernel_name = fmask.name("scan_k1_bitmap_kernel", "scan_k1_bitmap_kernel+filter", "scan_k1_bitmap_kernel+slots", "scan_k1_bitmap_kernel+tags", "scan_k1_bitmap_kernel+values", "scan_k1_bitmap_kernel+tags+values");
                hipLaunchKernelGGL((scan_k1_bitmap_kernel<CS, 4, decltype(m)...>), grid, block, 0, s, t.codes, t.norm_codes, luts,
                                   t.norm_table, p.segs, p.lpos, p.hdr, p.max_seg, nsplit, k64, so, m...);
                *did_select = so.ids != nullptr;
                return hipGetLastError();
            } else {
                *kernel_name = fmask.name("scan_k1_kernel", "scan_k1_kernel+filter", "scan_k1_kernel+slots", "scan_k1_kernel+tags", "scan_k1_kernel+values", "scan_k1_kernel+tags+values");
                if (p.max_seg <= 64)
                    return position(int_c<64>(), int_c<4>(), so);
                // nprobe 65..256 (the DEEP1B preset probes 128 lists): a 5 KB plan instead of 20 KB keeps 7 workgroups
                // per CU resident instead of 4
                if (p.max_seg <= 256)
                    return position(int_c<256>(), int_c<4>(), so);
                return position(int_c<1024>(), int_c<4>(), so);
            }
        });
    });
}

// ---------------------------------------------------------------------------------------------
// keys -> (distance, label): the winner's scan position is looked up in the plan (segments are in
// scan order, so vpos ascends) and the label read from this shard's id array.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void resolve_key(unsigned long long key, const IvfTables &t, const Seg *sq, uint32_t nseg,
                                            float *dist, long long *label)
{
    const uint32_t hiw = (uint32_t)(key >> 32), vpos = (uint32_t)key;
    if (key >= kKeyInit) {
        *dist = FLT_MAX;
        *label = -1;
        return;
    }
    *dist = orderable_f32(hiw);
    *label = -1;
    if (nseg == 0)
        return;
    uint32_t a = 0, b = nseg - 1; // last segment with seg.vpos <= vpos
    while (a < b) {
        const uint32_t mid = (a + b + 1) >> 1;
        if (sq[mid].vpos <= vpos)
            a = mid;
        else
            b = mid - 1;
    }
    const Seg sg = sq[a];
    if (vpos >= sg.vpos && vpos - sg.vpos < sg.len)
        *label = (long long)t.ids[sg.start + (vpos - sg.vpos)];
}

__global__ void select_kernel(IvfTables t, const Seg *__restrict__ segs, const PlanHdr *__restrict__ hdr, int max_seg,
                              const unsigned long long *__restrict__ keys, int nq, int k, float *__restrict__ dist,
                              long long *__restrict__ labels, long long *__restrict__ out_keys, int keys_signed)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (size_t)nq * k)
        return;
    const int q = (int)(i / k);
    unsigned long long key = keys[i];
    if (keys_signed)
        key ^= kSignFlip;
    float dv;
    long long lb;
    resolve_key(key, t, segs + (size_t)q * max_seg, hdr[q].nseg, &dv, &lb);
    dist[i] = dv;
    labels[i] = lb;
    if (out_keys)
        out_keys[i] = (long long)(key ^ kSignFlip);
}

hipError_t launch_select(hipStream_t s, const IvfTables &t, const PlanView &p, const uint64_t *keys, int k, float *dist,
                         int64_t *labels, int64_t *out_keys)
{
    const size_t n = (size_t)p.nq * k;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, p.segs, p.hdr, p.max_seg,
                       reinterpret_cast<const unsigned long long *>(keys), p.nq, k, dist,
                       reinterpret_cast<long long *>(labels), reinterpret_cast<long long *>(out_keys), 0);
    return hipGetLastError();
}

hipError_t launch_resolve(hipStream_t s, const IvfTables &t, const PlanView &p, const int64_t *skeys, int k, float *dist,
                          int64_t *labels)
{
    const size_t n = (size_t)p.nq * k;
    if (n == 0)
        return hipSuccess;
    hipLaunchKernelGGL(select_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, t, p.segs, p.hdr, p.max_seg,
                       reinterpret_cast<const unsigned long long *>(skeys), p.nq, k, dist,
                       reinterpret_cast<long long *>(labels), (long long *)nullptr, 1);
    return hipGetLastError();
}

// ---------------------------------------------------------------------------------------------
// Synthetic corpus: byte b of stream(seed) = byte (b % 8) of
// mix64(seed + (b / 8 + 1) * 0x9E3779B97F4A7C15); reproducible on the host with numpy.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ unsigned long long mix64(unsigned long long z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void fill_bytes_kernel(uint8_t *__restrict__ dst, size_t nwords, size_t nbytes, unsigned long long seed)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t w = (size_t)blockIdx.x * blockDim.x + threadIdx.x; w < nwords; w += stride) {
        const unsigned long long v = mix64(seed + (w + 1) * 0x9E3779B97F4A7C15ull);
        if ((w + 1) * 8 <= nbytes) {
            reinterpret_cast<unsigned long long *>(dst)[w] = v;
        } else {
            for (size_t b = w * 8; b < nbytes; b++)
                dst[b] = (uint8_t)(v >> (8 * (b & 7)));
        }
    }
}

hipError_t launch_fill_bytes(hipStream_t s, uint8_t *dst, size_t nbytes, uint64_t seed)
{
    if (nbytes == 0)
        return hipSuccess;
    const size_t nwords = (nbytes + 7) / 8;
    const unsigned grid = (unsigned)std::min<size_t>((nwords + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(fill_bytes_kernel, dim3(grid), dim3(256), 0, s, dst, nwords, nbytes, (unsigned long long)seed);
    return hipGetLastError();
}

// Sharded form: one workgroup per owned list; list c's bytes are the bytes of the unsharded stream at its GLOBAL
// offset, so a shard holds exactly the slice of the single-GPU corpus it owns.
__global__ void fill_lists_kernel(IvfTables t, uint8_t *__restrict__ codes, uint8_t *__restrict__ norm_codes,
                                  uint32_t *__restrict__ ids, unsigned long long seed_codes,
                                  unsigned long long seed_norms)
{
    const int cs4 = t.M / 4; // dwords per code
    for (uint32_t c = blockIdx.x; c < t.nc; c += gridDim.x) {
        const uint32_t l0 = t.loff[c];
        if (l0 == kNotOwned)
            continue;
        const unsigned long long g0 = t.goff[c], n = t.goff[c + 1] - g0;
        uint32_t *dst = reinterpret_cast<uint32_t *>(codes + (size_t)l0 * t.M);
        for (unsigned long long j = threadIdx.x; j < n * cs4; j += blockDim.x) {
            const unsigned long long k = g0 * cs4 + j; // global dword index of the code stream
            const unsigned long long v = mix64(seed_codes + ((k >> 1) + 1) * 0x9E3779B97F4A7C15ull);
            dst[j] = (uint32_t)(v >> (32 * (k & 1)));
        }
        for (unsigned long long j = threadIdx.x; j < n; j += blockDim.x) {
            const unsigned long long b = g0 + j;
            const unsigned long long v = mix64(seed_norms + ((b >> 3) + 1) * 0x9E3779B97F4A7C15ull);
            norm_codes[l0 + j] = (uint8_t)(v >> (8 * (b & 7)));
            ids[l0 + j] = (uint32_t)b;
        }
    }
}

hipError_t launch_fill_lists(hipStream_t s, const IvfTables &t, uint8_t *codes, uint8_t *norm_codes, uint32_t *ids,
                             uint64_t seed_codes, uint64_t seed_norms)
{
    hipLaunchKernelGGL(fill_lists_kernel, dim3(256 * 8), dim3(256), 0, s, t, codes, norm_codes, ids,
                       (unsigned long long)seed_codes, (unsigned long long)seed_norms);
    return hipGetLastError();
}

__global__ void fill_iota_kernel(uint32_t *__restrict__ dst, size_t n, uint32_t first)
{
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride)
        dst[i] = first + (uint32_t)i;
}

hipError_t launch_fill_iota(hipStream_t s, uint32_t *dst, size_t n, uint32_t first)
{
    if (n == 0)
        return hipSuccess;
    const unsigned grid = (unsigned)std::min<size_t>((n + 255) / 256, 256 * 16);
    hipLaunchKernelGGL(fill_iota_kernel, dim3(grid), dim3(256), 0, s, dst, n, first);
    return hipGetLastError();
}

__global__ void plan_totals_kernel(const PlanHdr *__restrict__ hdr, int nq, unsigned long long *out)
{
    unsigned long long tc = 0, ts = 0;
    for (int q = blockIdx.x * blockDim.x + threadIdx.x; q < nq; q += gridDim.x * blockDim.x) {
        tc += hdr[q].total;
        ts += hdr[q].nseg;
    }
    for (int off = 32; off >= 1; off >>= 1) {
        tc += __shfl_xor(tc, off, 64);
        ts += __shfl_xor(ts, off, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicAdd(&out[0], tc);
        atomicAdd(&out[1], ts);
    }
}

hipError_t launch_plan_totals(hipStream_t s, const PlanHdr *hdr, int nq, unsigned long long *out)
{
    hipError_t e = hipMemsetAsync(out, 0, 2 * sizeof(unsigned long long), s);
    if (e != hipSuccess || nq == 0)
        return e;
    hipLaunchKernelGGL(plan_totals_kernel, dim3(std::min((nq + 255) / 256, 256)), dim3(256), 0, s, hdr, nq, out);
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
