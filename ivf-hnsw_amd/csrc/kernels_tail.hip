// Everything behind the coarse stage in ONE launch, for small batches (IndexIVF_HNSW.cpp:262-293 for a handful of
// queries): the scan plan, the query's inner-product table, the ADC scan of its share of the plan, and -- by the last
// workgroup of a query to finish -- the label resolution and the result write.
//
// Why: one query per call is how the reference's drivers search (tests/test_ivfhnsw_sift1b.cpp:193-208).  plan_ivf_kernel,
// lut_kernel, scan_k1_kernel and select_kernel are four dependent launches of a few microseconds of work each; on an idle
// chip each costs ~7 us of dispatch and dependency latency (30 us of a 215 us call).  Here nq * nsplit workgroups each
// derive the (tiny) plan themselves, build the table from the L2-resident code book, scan their slice, and meet in one
// atomic per query.  Same arithmetic in the same order as the four kernels (plan rule of plan_ivf_kernel, ip_sse_order,
// the m-sequential ADC sum, packed (distance, scan position) keys), so the same bits.
//
// keys_inv[q] holds the bitwise complement of the best key (atomicMax; 0 = nothing yet, so a plain memset initialises
// it), done[q] counts finished workgroups of query q.
#include "plan_steps.h"
#include "scan_steps.h"

#include <float.h>

namespace ivfhnsw_gpu_impl {

namespace {

template <int CS, int DSUB, int U>
__global__ __launch_bounds__(256) void ivf_tail_kernel(IvfTables t, const float *__restrict__ xq,
                                                       const uint32_t *__restrict__ cid, const float *__restrict__ cd,
                                                       int nq, int nprobe, unsigned long long max_codes, int nsplit,
                                                       unsigned long long *__restrict__ keys_inv,
                                                       uint32_t *__restrict__ done, PlanHdr *__restrict__ hdr_out,
                                                       float *__restrict__ dist_out, long long *__restrict__ labels_out,
                                                       const uint32_t *__restrict__ status_word,
                                                       uint32_t *__restrict__ status_out)
{
    constexpr int D = CS * DSUB;
    __shared__ __attribute__((aligned(16))) float s_lut[CS * 256];
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) float s_x[D];
    __shared__ __attribute__((aligned(16))) Seg s_seg[64];
    __shared__ uint32_t s_lpos[65];
    __shared__ uint32_t s_nseg, s_last;
    __shared__ unsigned long long s_red[4];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / nsplit;
    const int split = blockIdx.x - q * nsplit;

    // ---- stage the query and the norm table; wave 0 derives the plan (plan_ivf_kernel for nprobe <= 64)
    if (tid < D)
        s_x[tid] = xq[(size_t)q * D + tid];
    s_norm[tid] = t.norm_table[tid];
    if (wave == 0) {
        PlanCursor cur;
        ivf_plan_chunk(cur, t, cid + (size_t)q * nprobe, cd + (size_t)q * nprobe, 0, nprobe, max_codes, s_seg, s_lpos, lane);
        const uint32_t ns = cur.ns, nl = cur.nl;
        if (lane == 0) {
            s_nseg = ns;
            s_lpos[ns] = nl;
            if (split == 0 && hdr_out) // the accounting of ivfhnsw_gpu_last_scan_counts
                store_plan_hdr(&hdr_out[q], ns, nl);
        }
    }
    __syncthreads();
    const uint32_t nseg = s_nseg;
    const uint32_t total = s_lpos[nseg];

    unsigned long long best = kKeyInit;
    const auto [lo, hi] = scan_slice(total, nsplit, split, 256);
    if (lo < hi) { // block-uniform
        // ---- table: thread c builds tab[m][c] for every m (lut_kernel's arithmetic; the code book comes from L2)
        {
            const int c = tid;
#pragma unroll 4
            for (int m = 0; m < CS; m++) {
                const float *src = t.pq_centroids + ((size_t)m * 256 + c) * DSUB;
                float row[DSUB];
                if constexpr (DSUB % 4 == 0) {
#pragma unroll
                    for (int i = 0; i < DSUB; i += 4) {
                        const float4 v = *reinterpret_cast<const float4 *>(src + i);
                        row[i] = v.x, row[i + 1] = v.y, row[i + 2] = v.z, row[i + 3] = v.w;
                    }
                } else {
#pragma unroll
                    for (int i = 0; i < DSUB; i += 2) {
                        const float2 v = *reinterpret_cast<const float2 *>(src + i);
                        row[i] = v.x, row[i + 1] = v.y;
                    }
                }
                s_lut[m * 256 + c] = ip_sse_order<DSUB>(s_x + m * DSUB, row, DSUB);
            }
        }
        __syncthreads();
        // ---- scan of [lo, hi): one plan chunk, walked as scan_k1_kernel walks it (scan_steps.h)
        SegCursor c;
        for (uint32_t base = lo; base < hi; base += 256 * U) {
            uint32_t w[U][CS / 4];
            uint32_t nb[U], vp[U];
            float ct[U];
            bool ok[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t p = base + u * 256 + tid;
                ok[u] = p < hi;
                if (ok[u]) {
                    c.seek<SeekLinear>(p, s_lpos, s_seg, nseg);
                    const uint32_t off = p - c.seg_lo;
                    const uint32_t gi = c.seg_start + off;
                    load_code_words<CS>(t.codes, gi, w[u]);
                    nb[u] = t.norm_codes[gi];
                    vp[u] = c.seg_vpos + off;
                    ct[u] = c.seg_ct;
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if (ok[u]) {
                    const float sum = adc_sum<CS>(s_lut, w[u]);
                    const float dist = adc_distance(ct[u], s_norm[nb[u]], sum);
                    if (dist < FLT_MAX) {
                        const unsigned long long key = adc_key(dist, vp[u]);
                        best = key < best ? key : best;
                    }
                }
            }
        }
    }
    best = wave_min_u64(best);
    if (lane == 0)
        s_red[wave] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned long long b = s_red[0];
#pragma unroll
        for (int i = 1; i < 4; i++)
            b = s_red[i] < b ? s_red[i] : b;
        if (b < kKeyInit)
            atomicMax(&keys_inv[q], ~b);
        __threadfence();
        s_last = atomicAdd(&done[q], 1u) == (uint32_t)nsplit - 1u ? 1u : 0u;
    }
    __syncthreads();
    if (!s_last || tid != 0)
        return;
    // ---- the last workgroup of the query: the winner's scan position -> label (the plan is still in LDS)
    __threadfence();
    const unsigned long long inv = atomicMax(&keys_inv[q], 0ull); // a read that sees the other workgroups' maxima
    const unsigned long long key = ~inv;
    float dv = FLT_MAX;
    long long lb = -1;
    if (inv != 0ull && key < kKeyInit) {
        dv = orderable_f32((uint32_t)(key >> 32));
        const uint32_t vpos = (uint32_t)key;
        for (uint32_t i = 0; i < nseg; i++) {
            const Seg sg = s_seg[i];
            if (vpos >= sg.vpos && vpos - sg.vpos < sg.len) {
                lb = (long long)t.ids[sg.start + (vpos - sg.vpos)];
                break;
            }
        }
    }
    dist_out[q] = dv;
    labels_out[q] = lb;
    if (q == 0 && status_out)
        *status_out = *status_word;
}

} // namespace

bool ivf_tail_supported(const IvfTables &t, int nprobe, int k)
{
    // IVFHNSW_TAIL=0 keeps the four launches (A/B runs)
    static const bool off = [] {
        const char *e = getenv("IVFHNSW_TAIL");
        return e && *e && atoi(e) == 0;
    }();
    if (off || k != 1 || nprobe > 64 || t.shard_world != 1)
        return false;
    return (t.M == 16 && (t.dsub == 8 || t.dsub == 6)) || (t.M == 8 && (t.dsub == 16 || t.dsub == 12));
}

hipError_t launch_ivf_tail(hipStream_t s, const IvfTables &t, const float *xq, const uint32_t *cid, const float *cd,
                           int nq, int nprobe, uint64_t max_codes, int nsplit, uint64_t *keys_inv, uint32_t *done,
                           PlanHdr *hdr, float *dist, int64_t *labels, const uint32_t *status_word, uint32_t *status_out)
{
    if (nq == 0)
        return hipSuccess;
    const dim3 grid((unsigned)nq * nsplit), block(256);
#define IVFHNSW_TAIL(CS, DSUB)                                                                                        \
    hipLaunchKernelGGL((ivf_tail_kernel<CS, DSUB, 4>), grid, block, 0, s, t, xq, cid, cd, nq, nprobe,                 \
                       (unsigned long long)max_codes, nsplit, reinterpret_cast<unsigned long long *>(keys_inv), done, \
                       hdr, dist, reinterpret_cast<long long *>(labels), status_word, status_out)
    if (t.M == 16 && t.dsub == 8)
        IVFHNSW_TAIL(16, 8);
    else if (t.M == 16 && t.dsub == 6)
        IVFHNSW_TAIL(16, 6);
    else if (t.M == 8 && t.dsub == 16)
        IVFHNSW_TAIL(8, 16);
    else if (t.M == 8 && t.dsub == 12)
        IVFHNSW_TAIL(8, 12);
    else
        return hipErrorInvalidValue;
#undef IVFHNSW_TAIL
    return hipGetLastError();
}

} // namespace ivfhnsw_gpu_impl
