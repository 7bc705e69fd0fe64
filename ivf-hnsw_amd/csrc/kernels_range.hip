// gfx950 kernels of range search: every scored code with dist < radius, in scan order.
//
// The scan of kernels_search.hip keeps a minimum; this one keeps hits.  Plan, table and filter mask are consumed by the
// steps scan_k1_kernel / scan_k1_bitmap_kernel consume them by (scan_steps.h), and the distance is adc_distance, so a
// returned distance is bit for bit what the k-search returns for that code.  Two passes over the same
// (query, slice) grid: COUNT leaves the hits of every slice, a prefix over them gives every slice its place in the
// output, FILL scores the slice again and writes hit number r of the slice at base + r.  A slice without hits ends the
// fill pass before it stages its table.
//
// Float contract as in kernels_search.hip: explicit round-to-nearest intrinsics, built with -ffp-contract=off.
#include "scan_steps.h"

#include <float.h>
#include <algorithm>

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_SEGCAP = 256; // plan segments staged at a time (position form)

struct RangeOut {
    const uint32_t *ids;
    float *dist;
    long long *labels;
};

// What a workgroup does with the hits of one tile: U rows of RG_THREADS consecutive positions, row u before row u + 1,
// lane t of a row before lane t + 1 -- position order.
// COUNT: run += the wavefront's hits (wave-uniform).
// FILL: the rank of a hit = hits of the slice before this tile (run, block-uniform) + hits of earlier rows + hits of
// earlier wavefronts in its row (s_wcnt, through LDS) + hits of earlier lanes in its wavefront (ballot + mbcnt).  One
// barrier per tile: s_wcnt is double buffered, a wavefront can run at most one barrier ahead of the slowest.
template <int U, bool FILL>
__device__ __forceinline__ void range_tile(const bool (&hit)[U], const float (&dv)[U], const uint32_t (&gi)[U],
                                           uint32_t (*s_wcnt)[U][RG_THREADS / 64], int &buf, uint32_t &run,
                                           uint32_t base, const RangeOut &out, int lane, int wave)
{
    if constexpr (!FILL) {
#pragma unroll
        for (int u = 0; u < U; u++)
            run += (uint32_t)__popcll(__ballot(hit[u]));
    } else {
        uint32_t rank[U];
#pragma unroll
        for (int u = 0; u < U; u++) {
            const unsigned long long b = __ballot(hit[u]);
            rank[u] = __builtin_amdgcn_mbcnt_hi((uint32_t)(b >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)b, 0u));
            if (lane == 0)
                s_wcnt[buf][u][wave] = (uint32_t)__popcll(b);
        }
        __syncthreads();
        uint32_t acc = run;
#pragma unroll
        for (int u = 0; u < U; u++) {
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < RG_THREADS / 64; w++) {
                const uint32_t c = s_wcnt[buf][u][w];
                before += w < wave ? c : 0u;
                all += c;
            }
            if (hit[u]) {
                const size_t pos = (size_t)base + acc + before + rank[u];
                out.dist[pos] = dv[u];
                out.labels[pos] = (long long)out.ids[gi[u]];
            }
            acc += all;
        }
        run = acc;
        buf ^= 1;
    }
}

// COUNT: slices[blockIdx.x] (zero before) += the hits of this (query, slice)
template <bool FILL>
__device__ __forceinline__ void range_finish(uint32_t *slices, uint32_t run, int lane)
{
    if constexpr (!FILL) {
        if (lane == 0 && run)
            atomicAdd(&slices[blockIdx.x], run);
    }
}

// Position form (whole inverted lists): scan_slice, stage_plan_chunk and a SegCursor, as scan_k1_kernel.
// CS == 0: run-time code size cs_rt, table in dynamic LDS.  Mask: empty, the pass mask of a label filter, or filter slots
// per query (device_common.h filter_mask).
template <int CS, int U, bool FILL, class... Mask>
__global__ __launch_bounds__(RG_THREADS) void range_scan_kernel(const uint8_t *__restrict__ codes,
                                                                const uint8_t *__restrict__ norm_codes,
                                                                const float *__restrict__ luts,
                                                                const float *__restrict__ norm_table,
                                                                const Seg *__restrict__ segs,
                                                                const uint32_t *__restrict__ lpos,
                                                                const PlanHdr *__restrict__ hdr, int max_seg, int nsplit,
                                                                int cs_rt, float radius, uint32_t *slices, RangeOut out,
                                                                Mask... fmask_arg)
{
    constexpr bool FILT = sizeof...(Mask) != 0;
    constexpr int FK = filter_kind<Mask...>;
    __shared__ __attribute__((aligned(16))) float s_lut_fixed[(CS > 0 ? CS : 1) * 256];
    extern __shared__ __attribute__((aligned(16))) float s_lut_dyn[];
    float *s_lut = CS > 0 ? s_lut_fixed : s_lut_dyn;
    const int csz = CS > 0 ? CS : cs_rt;
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) Seg s_seg[RG_SEGCAP];
    __shared__ uint32_t s_lpos[RG_SEGCAP + 1];
    __shared__ uint32_t s_wcnt[2][U][RG_THREADS / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / nsplit;
    [[maybe_unused]] FilterFill ffill; // filter slots: what a query without a plane reads instead (filter_mask)
    [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(q, ffill, fmask_arg...);
    const int split = blockIdx.x - q * nsplit;
    const PlanHdr h = hdr[q];
    if (h.total == 0)
        return;
    const auto [lo, hi] = scan_slice(h.total, nsplit, split, RG_THREADS);
    if (lo >= hi)
        return;
    uint32_t out_base = 0;
    if constexpr (FILL) {
        out_base = slices[blockIdx.x];
        if (slices[blockIdx.x + 1] == out_base) // the count pass found nothing here
            return;
    }
    stage_table_dma<RG_THREADS>(luts, q, csz, s_lut, tid);
    s_norm[tid] = norm_table[tid];

    const Seg *sq = segs + (size_t)q * max_seg;
    const uint32_t *lq = lpos + (size_t)q * max_seg;
    uint32_t run = 0;
    int buf = 0;

    for (uint32_t cs = 0; cs < h.nseg; cs += RG_SEGCAP) {
        const uint32_t cn = min((uint32_t)RG_SEGCAP, h.nseg - cs);
        const uint32_t ch = plan_chunk_end(lq, cs, cn, h.nseg, h.total);
        if (ch <= lo) // block-uniform: the chunk ends before this slice
            continue;
        if (lq[cs] >= hi)
            break;
        __syncthreads(); // previous chunk fully consumed (and the tables staged, first time)
        stage_plan_chunk<RG_THREADS>(sq, lq, cs, cn, ch, s_seg, s_lpos, tid);
        __syncthreads();
        const uint32_t cl = s_lpos[0];
        const uint32_t b0 = max(cl, lo), b1 = min(ch, hi);
        SegCursor c;
        for (uint32_t base = b0; base < b1; base += RG_THREADS * U) {
            CodeRegs<CS> w[U];
            uint32_t nb[U], gi[U];
            [[maybe_unused]] FilterWord<FK> fw[U];
            float ct[U], dv[U];
            bool ok[U], hit[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t p = base + u * RG_THREADS + tid;
                ok[u] = p < b1;
                gi[u] = 0;
                if (ok[u]) {
                    c.seek<SeekStep2Halves>(p, s_lpos, s_seg, cn);
                    gi[u] = c.seg_start + (p - c.seg_lo);
                    code_fetch<CS>(codes, gi[u], cs_rt, s_lut, w[u]);
                    load_norm_filter<FK>(norm_codes, fmask, gi[u], nb[u], fw[u], ffill);
                    ct[u] = c.seg_ct;
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if constexpr (FILT)
                    ok[u] = ok[u] && filter_pass<FK>(fw[u], gi[u] & 31u, ffill);
                hit[u] = false;
                dv[u] = 0.f;
                if (ok[u]) {
                    const float sum = code_sum_lds<CS>(s_lut, w[u]);
                    const float dist = adc_distance(ct[u], s_norm[nb[u]], sum);
                    hit[u] = dist < radius; // strict, and false for a NaN distance
                    dv[u] = adc_value(dist);
                }
            }
            range_tile<U, FILL>(hit, dv, gi, s_wcnt, buf, run, out_base, out, lane, wave);
        }
    }
    range_finish<FILL>(slices, run, lane);
}

// Short-segment form (Grouping sub-groups of ~10-16 codes): positions are dealt to lanes one code each and the segment of
// a position comes from a bitmap of segment starts plus the starts before every 64-position word (scan_steps.h
// BitmapChunk, as scan_k1_bitmap_kernel) -- one broadcast LDS read and two v_mbcnt instead of a search per position.
template <int CS, int U, bool FILL, class... Mask>
__global__ __launch_bounds__(RG_THREADS) void range_scan_bitmap_kernel(const uint8_t *__restrict__ codes,
                                                                       const uint8_t *__restrict__ norm_codes,
                                                                       const float *__restrict__ luts,
                                                                       const float *__restrict__ norm_table,
                                                                       const Seg *__restrict__ segs,
                                                                       const uint32_t *__restrict__ lpos,
                                                                       const PlanHdr *__restrict__ hdr, int max_seg,
                                                                       int nsplit, float radius, uint32_t *slices,
                                                                       RangeOut out, Mask... fmask_arg)
{
    constexpr bool FILT = sizeof...(Mask) != 0;
    constexpr int FK = filter_kind<Mask...>;
    __shared__ __attribute__((aligned(16))) float s_lut[CS * 256];
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) Seg s_seg[kBmSegCap];
    __shared__ uint32_t s_lpos[kBmSegCap + 1];
    __shared__ unsigned long long s_mask[kBmSpanWords];
    __shared__ uint32_t s_pref[kBmSpanWords];
    __shared__ uint32_t s_wtot[RG_THREADS / 64];
    __shared__ uint32_t s_wcnt[2][U][RG_THREADS / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / nsplit;
    [[maybe_unused]] FilterFill ffill; // filter slots: what a query without a plane reads instead (filter_mask)
    [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(q, ffill, fmask_arg...);
    const int split = blockIdx.x - q * nsplit;
    const PlanHdr h = hdr[q];
    if (h.total == 0)
        return;
    const auto [lo, hi] = scan_slice(h.total, nsplit, split, RG_THREADS);
    if (lo >= hi)
        return;
    uint32_t out_base = 0;
    if constexpr (FILL) {
        out_base = slices[blockIdx.x];
        if (slices[blockIdx.x + 1] == out_base)
            return;
    }
    stage_table_dma<RG_THREADS>(luts, q, CS, s_lut, tid);
    s_norm[tid] = norm_table[tid];

    const Seg *sq = segs + (size_t)q * max_seg;
    const uint32_t *lq = lpos + (size_t)q * max_seg;
    uint32_t run = 0;
    int buf = 0;

    uint32_t cs = first_segment(lq, h.nseg, lo);
    while (cs < h.nseg) {
        const uint32_t cl = lq[cs];
        if (cl >= hi)
            break;
        const BitmapChunk bc =
            stage_bitmap_chunk<RG_THREADS>(sq, lq, cs, h.nseg, h.total, s_seg, s_lpos, s_mask, s_pref, s_wtot, tid);
        const uint32_t b0 = max(cl, lo), b1 = min(bc.ch, hi);
        if (b0 < b1) {
            for (uint32_t rbase = (b0 - cl) & ~63u; rbase < b1 - cl; rbase += RG_THREADS * U) {
                CodeRegs<CS> w[U];
                uint32_t nb[U], gi[U];
                [[maybe_unused]] FilterWord<FK> fw[U];
                float ct[U], dv[U];
                bool ok[U], hit[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t r = rbase + u * RG_THREADS + tid;
                    const uint32_t p = cl + r;
                    ok[u] = p >= b0 && p < b1;
                    gi[u] = 0;
                    const uint32_t wi = BitmapChunk::word_of(r);
                    if (wi * 64u < b1 - cl) { // wave-uniform
                        const uint32_t sgi = bc.segment_of(wi, lane);
                        if (ok[u]) {
                            const Seg sg = s_seg[sgi];
                            gi[u] = sg.start + (p - s_lpos[sgi]);
                            code_fetch<CS>(codes, gi[u], CS, s_lut, w[u]);
                            load_norm_filter<FK>(norm_codes, fmask, gi[u], nb[u], fw[u], ffill);
                            ct[u] = sg.cterm;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if constexpr (FILT)
                        ok[u] = ok[u] && filter_pass<FK>(fw[u], gi[u] & 31u, ffill);
                    hit[u] = false;
                    dv[u] = 0.f;
                    if (ok[u]) {
                        const float sum = code_sum_lds<CS>(s_lut, w[u]);
                        const float dist = adc_distance(ct[u], s_norm[nb[u]], sum);
                        hit[u] = dist < radius;
                        dv[u] = adc_value(dist);
                    }
                }
                range_tile<U, FILL>(hit, dv, gi, s_wcnt, buf, run, out_base, out, lane, wave);
            }
        }
        cs += bc.cn;
    }
    range_finish<FILL>(slices, run, lane);
}

// lims[q] = the place of query q's first slice (bases: the exclusive scan of the slice counts, [nq * nsplit + 1])
__global__ void range_lims_kernel(const uint32_t *__restrict__ bases, int nq, int nsplit, unsigned long long *__restrict__ lims)
{
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q <= nq)
        lims[q] = bases[(size_t)q * nsplit];
}

// *out (zero before) += the 64-bit sum of counts [len]: the batch total before the 32-bit prefix is taken
__global__ void range_total_kernel(const uint32_t *__restrict__ counts, size_t len, unsigned long long *out)
{
    unsigned long long t = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < len; i += (size_t)gridDim.x * blockDim.x)
        t += counts[i];
    for (int off = 32; off >= 1; off >>= 1)
        t += __shfl_xor(t, off, 64);
    if ((threadIdx.x & 63) == 0 && t)
        atomicAdd(out, t);
}

template <bool FILL>
hipError_t range_launch(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int nsplit, int seg_len_hint,
                        float radius, uint32_t *slices, RangeOut out, const ScanFilter &fmask, const char **name)
{
    const dim3 grid((unsigned)p.nq * nsplit), block(RG_THREADS);
    return by_code_size<4, 8, 16, 32>(t.M, [&](auto cs) {
        return with_mask(fmask, [&](auto... m) -> hipError_t {
            constexpr int CS = decltype(cs)::value;
            if constexpr (CS > 0) {
                // plans of short segments (Grouping sub-groups): the bitmap form; whole lists: the position form
                if (seg_len_hint > 0 && seg_len_hint <= 48) {
                    *name = fmask.name("range_scan_bitmap_kernel", "range_scan_bitmap_kernel+filter", "range_scan_bitmap_kernel+slots", "range_scan_bitmap_kernel+tags", "range_scan_bitmap_kernel+values", "range_scan_bitmap_kernel+tags+values");
                    hipLaunchKernelGGL((range_scan_bitmap_kernel<CS, 4, FILL, decltype(m)...>), grid, block, 0, s, t.codes,
                                       t.norm_codes, luts, t.norm_table, p.segs, p.lpos, p.hdr, p.max_seg, nsplit, radius, slices,
                                       out, m...);
                    return hipGetLastError();
                }
            }
            // a compiled size unrolls by 4; any other multiple of 4 (IndexIVF_HNSW.cpp:805) is the run-time form, by 2
            constexpr auto kern = range_scan_kernel<CS, (CS > 0 ? 4 : 2), FILL, decltype(m)...>;
            size_t shm;
            if (hipError_t e = scan_table_lds<CS, kern>(t.M, &shm); e != hipSuccess)
                return e;
            *name = CS > 0 ? fmask.name("range_scan_kernel", "range_scan_kernel+filter", "range_scan_kernel+slots", "range_scan_kernel+tags", "range_scan_kernel+values", "range_scan_kernel+tags+values")
                           : fmask.name("range_scan_kernel (run-time code size)", "range_scan_kernel (run-time code size)+filter",
                                        "range_scan_kernel (run-time code size)+slots", "range_scan_kernel (run-time code size)+tags", "range_scan_kernel (run-time code size)+values", "range_scan_kernel (run-time code size)+tags+values");
            hipLaunchKernelGGL(kern, grid, block, shm, s, t.codes, t.norm_codes, luts, t.norm_table, p.segs, p.lpos, p.hdr,
                               p.max_seg, nsplit, t.M, radius, slices, out, m...);
            return hipGetLastError();
        });
    });
}

} // namespace

hipError_t launch_range_count(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int nsplit,
                              int seg_len_hint, float radius, uint32_t *slices, unsigned long long *total,
                              const ScanFilter &fmask, const char **kernel_name)
{
    const char *unused_name;
    kernel_name = kernel_name ? kernel_name : &unused_name; // may be null
    *kernel_name = "";
    const size_t len = (size_t)p.nq * nsplit + 1;
    hipError_t e = hipMemsetAsync(slices, 0, len * sizeof(uint32_t), s);
    if (e == hipSuccess)
        e = hipMemsetAsync(total, 0, sizeof(unsigned long long), s);
    if (e != hipSuccess || p.nq == 0)
        return e;
    e = range_launch<false>(s, t, luts, p, nsplit, seg_len_hint, radius, slices, RangeOut{nullptr, nullptr, nullptr}, fmask,
                            kernel_name);
    if (e != hipSuccess)
        return e;
    const unsigned grid = (unsigned)std::min<size_t>((len + 255) / 256, 1024);
    hipLaunchKernelGGL(range_total_kernel, dim3(grid), dim3(256), 0, s, slices, len, total);
    return hipGetLastError();
}

hipError_t launch_range_lims(hipStream_t s, const uint32_t *bases, int nq, int nsplit, uint64_t *lims)
{
    hipLaunchKernelGGL(range_lims_kernel, dim3((unsigned)(nq + 256) / 256), dim3(256), 0, s, bases, nq, nsplit,
                       reinterpret_cast<unsigned long long *>(lims));
    return hipGetLastError();
}

hipError_t launch_range_fill(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int nsplit,
                             int seg_len_hint, float radius, const uint32_t *bases, float *dist, int64_t *labels,
                             const ScanFilter &fmask)
{
    if (p.nq == 0)
        return hipSuccess;
    const char *name = "";
    return range_launch<true>(s, t, luts, p, nsplit, seg_len_hint, radius, const_cast<uint32_t *>(bases),
                              RangeOut{t.ids, dist, reinterpret_cast<long long *>(labels)}, fmask, &name);
}

} // namespace ivfhnsw_gpu_impl
