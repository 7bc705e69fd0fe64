// k > 1 in faiss heap-array order with no bound on k and none on the codes the heap admits (IndexIVF_HNSW.cpp:265,
// 285-288).  heap_scan_kernel scores a query's codes straight from the plan and the table the search has built, by the
// steps of scan_topk_kernel (kernels_topk.hip, scan_steps.h), and replays the reference's pop/push over them itself: no
// candidate stream, so no stream cap.
//
// Exactness is the argument above heap_replay_kernel: a code that fails dist < distances[0] leaves the heap untouched, and
// a root read earlier in the scan is never below the current root.  So the codes of a chunk that pass dist < root, with
// root read when the chunk starts, are a superset of the codes the heap admits from that chunk, in scan order, and
// replaying them (strict '<' against the CURRENT root, values only) leaves the reference's heap array bit for bit.
//
// One 256-thread workgroup per query.  The heap is (value, scan position) pairs; labels are resolved for the k survivors
// at the end.  Two tiers, chosen per launch from k and the code size (heap_scan_lds_tier):
//   LDS     the heap beside the table and the chunk buffer (8 k bytes; k <~ 16 500 at PQ16, <~ 2 200 at code size 128)
//   global  the heap in a per-workgroup slot of a global workspace: exact but slow, every level of a sift is a round
//           trip to L2 (~200 cycles instead of ~50 for a dependent ds_read)
#include "scan_steps.h"

#include <float.h>

namespace ivfhnsw_gpu_impl {

constexpr int HS_U = 4;                // codes per thread per chunk
constexpr int HS_CHUNK = 256 * HS_U;   // codes scored between two replays
constexpr int HS_SEGCAP = 256;         // plan segments staged in LDS at a time
constexpr int HS_GRID_MAX = 1024;      // workgroups per launch (the launch walks its queries with a grid stride)
constexpr size_t HS_WS_MAX = 512ull << 20; // global tier: bound on the heap workspace (grid x 8 k bytes)
constexpr size_t HS_LDS = 160 * 1024;      // LDS of one workgroup on gfx950
// static LDS of the kernel (norm table, segments, chunk buffer, counts) with room for alignment
constexpr size_t HS_STATIC_LDS = 256 * 4 + HS_SEGCAP * sizeof(Seg) + (HS_SEGCAP + 1) * 4 + HS_CHUNK * 8 + HS_U * 4 * 4 + 512;

// Mask: empty, the pass mask of a label filter, or filter slots per query -- the plane is resolved for every query the
// workgroup walks (device_common.h filter_mask): a row whose bit is clear never reaches
// the heap.
template <int CS, bool LDS_HEAP, class... Mask>
__global__ __launch_bounds__(256) void heap_scan_kernel(IvfTables t, const float *__restrict__ luts,
                                                        const Seg *__restrict__ segs, const uint32_t *__restrict__ lpos,
                                                        const PlanHdr *__restrict__ hdr, int max_seg, int nq, int k,
                                                        uint32_t *__restrict__ redo_hdr,
                                                        const uint32_t *__restrict__ redo_list, float *__restrict__ heap_ws,
                                                        float *__restrict__ dist, long long *__restrict__ labels,
                                                        Mask... fmask_arg)
{
    constexpr bool FILT = sizeof...(Mask) != 0;
    constexpr int FK = filter_kind<Mask...>;
    // dynamic LDS: the query's table [csz][256], then (LDS tier) the heap's values [k] and scan positions [k]
    extern __shared__ __attribute__((aligned(16))) float s_dyn[];
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) Seg s_seg[HS_SEGCAP];
    __shared__ uint32_t s_lpos[HS_SEGCAP + 1];
    __shared__ float s_cd[HS_CHUNK];    // the chunk's candidates in scan order: value ...
    __shared__ uint32_t s_cp[HS_CHUNK]; // ... and scan position
    __shared__ uint32_t s_wcnt[HS_U][4];

    const int tid = threadIdx.x;
    const int csz = CS > 0 ? CS : t.M;
    float *s_lut = s_dyn;
    float *val = LDS_HEAP ? s_dyn + (size_t)csz * 256 : heap_ws + (size_t)blockIdx.x * 2 * k;
    uint32_t *hpos = reinterpret_cast<uint32_t *>(val + k);
    s_norm[tid] = t.norm_table[tid];
    // redo form: the queries heap_replay_kernel listed (the count is stable until the last workgroup below clears it)
    const uint32_t n = redo_list ? redo_hdr[0] : (uint32_t)nq;

    for (uint32_t item = blockIdx.x; item < n; item += gridDim.x) {
        const int q = redo_list ? (int)redo_list[item] : (int)item;
        [[maybe_unused]] FilterFill ffill; // filter slots: what a query without a plane reads instead (filter_mask)
        [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(q, ffill, fmask_arg...);
        const PlanHdr h = hdr[q];
        __syncthreads(); // the previous query's label pass is done with the heap
        for (int j = tid; j < k; j += 256) { // maxheap_heapify
            val[j] = FLT_MAX;
            hpos[j] = 0xffffffffu;
        }
        if (h.total) {
            const float4 *src = reinterpret_cast<const float4 *>(luts + (size_t)q * csz * 256);
            float4 *dst = reinterpret_cast<float4 *>(s_lut);
            for (int i = tid; i < csz * 64; i += 256)
                dst[i] = src[i];
        }
        const Seg *sq = segs + (size_t)q * max_seg;
        const uint32_t *lq = lpos + (size_t)q * max_seg;
        const uint32_t nseg = h.total ? h.nseg : 0u;
        for (uint32_t cs = 0; cs < nseg; cs += HS_SEGCAP) {
            const uint32_t cn = min((uint32_t)HS_SEGCAP, nseg - cs);
            const uint32_t ch = plan_chunk_end(lq, cs, cn, nseg, h.total);
            __syncthreads();
            stage_plan_chunk<256>(sq, lq, cs, cn, ch, s_seg, s_lpos, tid);
            __syncthreads();
            const uint32_t cl = s_lpos[0];
            SegCursor c;
            for (uint32_t base = cl; base < ch; base += HS_CHUNK) {
                const float root = val[0]; // the heap is at rest here (barrier behind the last replay)
                CodeRegs<CS> w[HS_U];
                uint32_t nbv[HS_U], vp[HS_U];
                [[maybe_unused]] FilterWord<FK> fw[HS_U];
                [[maybe_unused]] uint32_t fb[HS_U];
                float ct[HS_U], dn[HS_U];
                bool ok[HS_U], pass[HS_U];
#pragma unroll
                for (int u = 0; u < HS_U; u++) {
                    const uint32_t p = base + u * 256 + tid;
                    ok[u] = p < ch;
                    if (ok[u]) {
                        c.seek<SeekHalves>(p, s_lpos, s_seg, cn);
                        const uint32_t off = p - c.seg_lo;
                        const uint32_t gi = c.seg_start + off;
                        code_fetch<CS>(t.codes, gi, t.M, s_lut, w[u]);
                        load_norm_filter<FK>(t.norm_codes, fmask, gi, nbv[u], fw[u], ffill);
                        if constexpr (FILT)
                            fb[u] = gi & 31u;
                        vp[u] = c.seg_vpos + off;
                        ct[u] = c.seg_ct;
                    }
                }
#pragma unroll
                for (int u = 0; u < HS_U; u++) {
                    pass[u] = false;
                    dn[u] = 0.f;
                    if constexpr (FILT)
                        ok[u] = ok[u] && filter_pass<FK>(fw[u], fb[u], ffill);
                    if (ok[u]) {
                        const float sum = code_sum<CS>(s_lut, w[u]);
                        const float d = adc_distance(ct[u], s_norm[nbv[u]], sum);
                        if (d < FLT_MAX) {
                            dn[u] = adc_value(d);
                            pass[u] = dn[u] < root;
                        }
                    }
                }
                // compact the candidates in scan order (unroll step, then wave, then lane)
                unsigned long long bal[HS_U];
#pragma unroll
                for (int u = 0; u < HS_U; u++) {
                    bal[u] = __ballot(pass[u]);
                    if ((tid & 63) == 0)
                        s_wcnt[u][tid >> 6] = (uint32_t)__popcll(bal[u]);
                }
                __syncthreads();
                uint32_t total = 0, mine[HS_U];
#pragma unroll
                for (int u = 0; u < HS_U; u++) {
                    mine[u] = total;
#pragma unroll
                    for (int w2 = 0; w2 < 4; w2++) {
                        const uint32_t c = s_wcnt[u][w2];
                        if (w2 < (tid >> 6))
                            mine[u] += c;
                        total += c;
                    }
                }
#pragma unroll
                for (int u = 0; u < HS_U; u++)
                    if (pass[u]) {
                        const uint32_t i = mine[u] + (uint32_t)__popcll(bal[u] & ((1ull << (tid & 63)) - 1ull));
                        s_cd[i] = dn[u];
                        s_cp[i] = vp[u];
                    }
                __syncthreads();
                if (tid == 0)
                    for (uint32_t i = 0; i < total; i++) {
                        const float d = s_cd[i];
                        if (d < val[0])
                            heap_replace_top<uint32_t>(k, val, hpos, d, s_cp[i]);
                    }
                __syncthreads();
            }
        }
        __syncthreads();
        // labels of the survivors (segments ascend in vpos)
        float *out_d = dist + (size_t)q * k;
        long long *out_l = labels + (size_t)q * k;
        for (int j = tid; j < k; j += 256) {
            const uint32_t vpos = hpos[j];
            long long lab = -1;
            if (vpos != 0xffffffffu && h.nseg) {
                uint32_t a = 0, b = h.nseg - 1;
                while (a < b) {
                    const uint32_t mid = (a + b + 1) >> 1;
                    if (sq[mid].vpos <= vpos)
                        a = mid;
                    else
                        b = mid - 1;
                }
                const Seg sg = sq[a];
                lab = (long long)t.ids[sg.start + (vpos - sg.vpos)];
            }
            out_d[j] = val[j];
            out_l[j] = lab;
        }
    }
    if (redo_list) {
        // the last workgroup out leaves the list's header zero for the next search (no memset on the stream)
        __syncthreads();
        if (tid == 0) {
            __threadfence();
            if (atomicAdd(&redo_hdr[1], 1u) == gridDim.x - 1) {
                redo_hdr[0] = 0;
                redo_hdr[1] = 0;
            }
        }
    }
}

bool heap_scan_lds_tier(int code_size, int k)
{
    return HS_STATIC_LDS + (size_t)code_size * 1024 + (size_t)8 * k <= HS_LDS;
}

static int heap_scan_grid(int code_size, int k, int nq)
{
    size_t g = std::min<size_t>((size_t)nq, HS_GRID_MAX);
    if (!heap_scan_lds_tier(code_size, k))
        g = std::min(g, HS_WS_MAX / ((size_t)8 * k));
    return (int)std::max<size_t>(g, 1);
}

size_t heap_scan_ws_bytes(int code_size, int k, int nq)
{
    return heap_scan_lds_tier(code_size, k) ? 0 : (size_t)heap_scan_grid(code_size, k, nq) * 8 * k;
}

hipError_t launch_heap_scan(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int k,
                            uint32_t *redo_hdr, const uint32_t *redo_list, float *heap_ws, float *dist, int64_t *labels,
                            const ScanFilter &fmask)
{
    if (p.nq == 0)
        return hipSuccess;
    if (k < 1 || !runtime_code_size_ok(t.M) || (redo_list && !redo_hdr))
        return hipErrorInvalidValue;
    const bool lds = heap_scan_lds_tier(t.M, k);
    if (!lds && !heap_ws)
        return hipErrorInvalidValue;
    // table and (LDS tier) heap are dynamic LDS at every code size; 0 = any other multiple of 4, the run-time form
    const size_t shm = (size_t)t.M * 1024 + (lds ? (size_t)8 * k : 0);
    const dim3 grid((unsigned)heap_scan_grid(t.M, k, p.nq)), block(256);
    return by_code_size<4, 8, 16, 32>(t.M, [&](auto cs) {
        return with_mask(fmask, [&](auto... m) {
            auto launch = [&](auto lds_heap) -> hipError_t {
                constexpr auto kern = heap_scan_kernel<decltype(cs)::value, decltype(lds_heap)::value, decltype(m)...>;
                if (hipError_t e = dyn_lds<kern>(shm); e != hipSuccess)
                    return e;
                hipLaunchKernelGGL(kern, grid, block, shm, s, t, luts, p.segs, p.lpos, p.hdr, p.max_seg, p.nq, k, redo_hdr,
                                   redo_list, heap_ws, dist, reinterpret_cast<long long *>(labels), m...);
                return hipGetLastError();
            };
            return lds ? launch(std::true_type()) : launch(std::false_type());
        });
    });
}

} // namespace ivfhnsw_gpu_impl
