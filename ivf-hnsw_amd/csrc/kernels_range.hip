// gfx950 kernels of range search: every scored code with dist < radius, in scan order.
//
// The scan of kernels_search.hip keeps a minimum; this one keeps hits.  Plan, table and filter mask are consumed exactly
// as scan_k1_kernel / scan_k1_bitmap_kernel consume them, and the distance is formed by the same intrinsics in the same
// order, so a returned distance is bit for bit what the k-search returns for that code.  Two passes over the same
// (query, slice) grid: COUNT leaves the hits of every slice, a prefix over them gives every slice its place in the
// output, FILL scores the slice again and writes hit number r of the slice at base + r.  A slice without hits ends the
// fill pass before it stages its table.
//
// Float contract as in kernels_search.hip: explicit round-to-nearest intrinsics, built with -ffp-contract=off.
#include "ivfhnsw_kernels.h"
#include "device_common.h"

#include <float.h>
#include <algorithm>

namespace ivfhnsw_gpu_impl {

namespace {

constexpr int RG_THREADS = 256;
constexpr int RG_SEGCAP = 256;                // plan segments staged at a time (position form)
constexpr int RG_BM_SEGCAP = 256;             // ... and in the bitmap form, whose chunk also spans at most
constexpr int RG_BM_SPANCAP = 8192;           // ... this many positions
constexpr int RG_BM_SPANW = RG_BM_SPANCAP / 64;

struct RangeOut {
    const uint32_t *ids;
    float *dist;
    long long *labels;
};

// the ADC sum of one code, m = 0..CS-1 in order (IndexIVF_HNSW.cpp:802-814); byte-offset table addressing as the k = 1
// scan's adc_sum_lds, the run-time form's sum was taken while the code was read (code_fetch)
template <int CS> __device__ __forceinline__ float range_code_sum(const float *s_lut, const CodeRegs<CS> &r)
{
    if constexpr (CS > 0) {
        float sum = 0.0f;
        const char *base = reinterpret_cast<const char *>(s_lut);
#pragma unroll
        for (int m = 0; m < CS; m++) {
            const uint32_t e = (r.w[m >> 2] >> ((m & 3) * 8)) & 0xffu;
            sum = __fadd_rn(sum, *reinterpret_cast<const float *>(base + m * 1024 + (e << 2)));
        }
        return sum;
    } else {
        return r.sum;
    }
}

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

// The table of query q into LDS, global -> LDS directly (global_load_lds_dwordx4: wave-uniform LDS base + lane * 16), and
// the norm table; the caller's next __syncthreads waits for both.
__device__ __forceinline__ void range_stage_tables(const float *luts, const float *norm_table, int q, int csz, float *s_lut,
                                                   float *s_norm, int tid)
{
    const float4 *src = reinterpret_cast<const float4 *>(luts + (size_t)q * csz * 256);
    const int lane = tid & 63;
    for (int i = tid; i < csz * 64; i += RG_THREADS)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i),
                                         (__attribute__((address_space(3))) void *)(reinterpret_cast<float4 *>(s_lut) + (i - lane)),
                                         16, 0, 0);
    s_norm[tid] = norm_table[tid];
}

// Position form (whole inverted lists): the slicing, the plan chunks and the per-lane segment cache of scan_k1_kernel.
// CS == 0: run-time code size cs_rt, table in dynamic LDS.  Mask: empty, or the pass mask of a label filter.
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
    [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(fmask_arg...);
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
    const int split = blockIdx.x - q * nsplit;
    const PlanHdr h = hdr[q];
    if (h.total == 0)
        return;
    // this slice of the query's virtual code array, in multiples of the block width
    uint32_t per = (h.total + nsplit - 1) / nsplit;
    per = (per + (RG_THREADS - 1)) & ~(uint32_t)(RG_THREADS - 1);
    const uint32_t lo = min((uint32_t)split * per, h.total);
    const uint32_t hi = min(lo + per, h.total);
    if (lo >= hi)
        return;
    uint32_t out_base = 0;
    if constexpr (FILL) {
        out_base = slices[blockIdx.x];
        if (slices[blockIdx.x + 1] == out_base) // the count pass found nothing here
            return;
    }
    range_stage_tables(luts, norm_table, q, csz, s_lut, s_norm, tid);

    const Seg *sq = segs + (size_t)q * max_seg;
    const uint32_t *lq = lpos + (size_t)q * max_seg;
    uint32_t run = 0;
    int buf = 0;

    for (uint32_t cs = 0; cs < h.nseg; cs += RG_SEGCAP) {
        const uint32_t cn = min((uint32_t)RG_SEGCAP, h.nseg - cs);
        const uint32_t ch = (cs + cn == h.nseg) ? h.total : lq[cs + cn];
        if (ch <= lo) // block-uniform: the chunk ends before this slice
            continue;
        if (lq[cs] >= hi)
            break;
        __syncthreads(); // previous chunk fully consumed (and the tables staged, first time)
        for (uint32_t i = tid; i < cn; i += RG_THREADS) {
            s_seg[i] = sq[cs + i];
            s_lpos[i] = lq[cs + i];
        }
        if (tid == 0)
            s_lpos[cn] = ch;
        __syncthreads();
        const uint32_t cl = s_lpos[0];
        const uint32_t b0 = max(cl, lo), b1 = min(ch, hi);
        // the segment this lane is inside, in registers: positions only grow, the LDS plan is searched again only when a
        // position runs past the segment's end
        uint32_t s = 0;
        uint32_t seg_lo = 0, seg_hi = 0, seg_start = 0;
        float seg_ct = 0.f;
        for (uint32_t base = b0; base < b1; base += RG_THREADS * U) {
            CodeRegs<CS> w[U];
            uint32_t nb[U], gi[U];
            [[maybe_unused]] uint32_t fw[U];
            float ct[U], dv[U];
            bool ok[U], hit[U];
#pragma unroll
            for (int u = 0; u < U; u++) {
                const uint32_t p = base + u * RG_THREADS + tid;
                ok[u] = p < b1;
                gi[u] = 0;
                if (ok[u]) {
                    if (p >= seg_hi) {
                        // first s with s_lpos[s + 1] > p, searched in [s, cn): two steps forward, then by halves
                        uint32_t a = s, b = cn - 1;
                        if (a < b && s_lpos[a + 1] <= p) {
                            a++;
                            if (a < b && s_lpos[a + 1] <= p)
                                a++;
                            else
                                b = a;
                        } else {
                            b = a;
                        }
                        while (a < b) {
                            const uint32_t mid = (a + b) >> 1;
                            if (s_lpos[mid + 1] > p)
                                b = mid;
                            else
                                a = mid + 1;
                        }
                        s = a;
                        const Seg sg = s_seg[s];
                        seg_lo = s_lpos[s];
                        seg_hi = seg_lo + sg.len;
                        seg_start = sg.start;
                        seg_ct = sg.cterm;
                    }
                    gi[u] = seg_start + (p - seg_lo);
                    code_fetch<CS>(codes, gi[u], cs_rt, s_lut, w[u]);
                    nb[u] = norm_codes[gi[u]];
                    if constexpr (FILT)
                        fw[u] = fmask[gi[u] >> 5];
                    ct[u] = seg_ct;
                }
            }
#pragma unroll
            for (int u = 0; u < U; u++) {
                if constexpr (FILT)
                    ok[u] = ok[u] && ((fw[u] >> (gi[u] & 31u)) & 1u);
                hit[u] = false;
                dv[u] = 0.f;
                if (ok[u]) {
                    const float sum = range_code_sum<CS>(s_lut, w[u]);
                    const float tt = __fadd_rn(ct[u], s_norm[nb[u]]);
                    const float dist = __fsub_rn(tt, __fmul_rn(2.0f, sum));
                    hit[u] = dist < radius; // strict, and false for a NaN distance
                    dv[u] = __fadd_rn(dist, 0.0f);
                }
            }
            range_tile<U, FILL>(hit, dv, gi, s_wcnt, buf, run, out_base, out, lane, wave);
        }
    }
    range_finish<FILL>(slices, run, lane);
}

// Short-segment form (Grouping sub-groups of ~10-16 codes): positions are dealt to lanes one code each and the segment of
// a position comes from a bitmap of segment starts plus the starts before every 64-position word, as in
// scan_k1_bitmap_kernel -- one broadcast LDS read and two v_mbcnt instead of a search per position, and no idle lanes.
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
    [[maybe_unused]] const uint32_t *__restrict__ fmask = filter_mask(fmask_arg...);
    __shared__ __attribute__((aligned(16))) float s_lut[CS * 256];
    __shared__ float s_norm[256];
    __shared__ __attribute__((aligned(16))) Seg s_seg[RG_BM_SEGCAP];
    __shared__ uint32_t s_lpos[RG_BM_SEGCAP + 1];
    __shared__ unsigned long long s_mask[RG_BM_SPANW];
    __shared__ uint32_t s_pref[RG_BM_SPANW];
    __shared__ uint32_t s_wtot[RG_THREADS / 64];
    __shared__ uint32_t s_wcnt[2][U][RG_THREADS / 64];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x / nsplit;
    const int split = blockIdx.x - q * nsplit;
    const PlanHdr h = hdr[q];
    if (h.total == 0)
        return;
    uint32_t per = (h.total + nsplit - 1) / nsplit;
    per = (per + 255u) & ~255u;
    const uint32_t lo = min((uint32_t)split * per, h.total);
    const uint32_t hi = min(lo + per, h.total);
    if (lo >= hi)
        return;
    uint32_t out_base = 0;
    if constexpr (FILL) {
        out_base = slices[blockIdx.x];
        if (slices[blockIdx.x + 1] == out_base)
            return;
    }
    range_stage_tables(luts, norm_table, q, CS, s_lut, s_norm, tid);

    const Seg *sq = segs + (size_t)q * max_seg;
    const uint32_t *lq = lpos + (size_t)q * max_seg;
    uint32_t run = 0;
    int buf = 0;

    // first segment of this slice: the last one starting at or before lo
    uint32_t cs = 0;
    if (lo > 0) {
        uint32_t a = 0, b = h.nseg - 1;
        while (a < b) {
            const uint32_t mid = (a + b + 1) >> 1;
            if (lq[mid] <= lo)
                a = mid;
            else
                b = mid - 1;
        }
        cs = a;
    }
    while (cs < h.nseg) {
        const uint32_t cl = lq[cs];
        if (cl >= hi)
            break;
        // as many segments as fit the plan buffer AND the bitmap's span; one oversized segment goes alone
        uint32_t cn = min((uint32_t)RG_BM_SEGCAP, h.nseg - cs);
        {
            const uint32_t end_all = (cs + cn == h.nseg) ? h.total : lq[cs + cn];
            if (end_all - cl > (uint32_t)RG_BM_SPANCAP) {
                uint32_t a = 1, b = cn > 1 ? cn - 1 : 1; // largest count whose end stays inside the span (or 1)
                while (a < b) {
                    const uint32_t mid = (a + b + 1) >> 1;
                    if (lq[cs + mid] - cl <= (uint32_t)RG_BM_SPANCAP)
                        a = mid;
                    else
                        b = mid - 1;
                }
                cn = a;
            }
        }
        const uint32_t ch = (cs + cn == h.nseg) ? h.total : lq[cs + cn];
        const bool single = ch - cl > (uint32_t)RG_BM_SPANCAP; // cn == 1: every position belongs to segment 0
        const uint32_t nwords = single ? 0u : (ch - cl + 63) >> 6;
        __syncthreads(); // previous chunk fully consumed (and the tables staged, first time)
        for (uint32_t i = tid; i < cn; i += RG_THREADS) {
            s_seg[i] = sq[cs + i];
            s_lpos[i] = lq[cs + i];
        }
        if (tid < (int)nwords)
            s_mask[tid] = 0ull;
        __syncthreads();
        if (!single) {
            uint32_t *m32 = reinterpret_cast<uint32_t *>(s_mask);
            for (uint32_t i = tid; i < cn; i += RG_THREADS) {
                const uint32_t r = s_lpos[i] - cl;
                atomicOr(&m32[r >> 5], 1u << (r & 31));
            }
            __syncthreads();
            // starts before every word (at most 128 words: waves 0 and 1 scan, two totals)
            const uint32_t cnt = tid < (int)nwords ? (uint32_t)__popcll(s_mask[tid]) : 0u;
            const uint32_t inc = wave_incl_scan(cnt, lane);
            if (lane == 63)
                s_wtot[wave] = inc;
            __syncthreads();
            if (tid < (int)nwords)
                s_pref[tid] = (wave ? s_wtot[0] : 0u) + inc - cnt;
            __syncthreads();
        }
        const uint32_t b0 = max(cl, lo), b1 = min(ch, hi);
        if (b0 < b1) {
            for (uint32_t rbase = (b0 - cl) & ~63u; rbase < b1 - cl; rbase += RG_THREADS * U) {
                CodeRegs<CS> w[U];
                uint32_t nb[U], gi[U];
                [[maybe_unused]] uint32_t fw[U];
                float ct[U], dv[U];
                bool ok[U], hit[U];
#pragma unroll
                for (int u = 0; u < U; u++) {
                    const uint32_t r = rbase + u * RG_THREADS + tid;
                    const uint32_t p = cl + r;
                    ok[u] = p >= b0 && p < b1;
                    gi[u] = 0;
                    const uint32_t wi = __builtin_amdgcn_readfirstlane(r >> 6);
                    if (wi * 64u < b1 - cl) { // wave-uniform
                        uint32_t sgi = 0;
                        if (!single) {
                            const unsigned long long mw = s_mask[wi];
                            const uint32_t below =
                                __builtin_amdgcn_mbcnt_hi((uint32_t)(mw >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mw, 0u));
                            sgi = s_pref[wi] + below + (uint32_t)((mw >> lane) & 1ull) - 1u;
                        }
                        if (ok[u]) {
                            const Seg sg = s_seg[sgi];
                            gi[u] = sg.start + (p - s_lpos[sgi]);
                            code_fetch<CS>(codes, gi[u], CS, s_lut, w[u]);
                            nb[u] = norm_codes[gi[u]];
                            if constexpr (FILT)
                                fw[u] = fmask[gi[u] >> 5];
                            ct[u] = sg.cterm;
                        }
                    }
                }
#pragma unroll
                for (int u = 0; u < U; u++) {
                    if constexpr (FILT)
                        ok[u] = ok[u] && ((fw[u] >> (gi[u] & 31u)) & 1u);
                    hit[u] = false;
                    dv[u] = 0.f;
                    if (ok[u]) {
                        const float sum = range_code_sum<CS>(s_lut, w[u]);
                        const float tt = __fadd_rn(ct[u], s_norm[nb[u]]);
                        const float dist = __fsub_rn(tt, __fmul_rn(2.0f, sum));
                        hit[u] = dist < radius;
                        dv[u] = __fadd_rn(dist, 0.0f);
                    }
                }
                range_tile<U, FILL>(hit, dv, gi, s_wcnt, buf, run, out_base, out, lane, wave);
            }
        }
        cs += cn;
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
                        float radius, uint32_t *slices, RangeOut out, const uint32_t *fmask, const char **name)
{
    const dim3 grid((unsigned)p.nq * nsplit), block(RG_THREADS);
    return by_code_size<4, 8, 16, 32>(t.M, [&](auto cs) {
        return with_mask(fmask, [&](auto... m) -> hipError_t {
            constexpr int CS = decltype(cs)::value;
            constexpr bool FILT = sizeof...(m) != 0;
            if constexpr (CS > 0) {
                // plans of short segments (Grouping sub-groups): the bitmap form; whole lists: the position form
                if (seg_len_hint > 0 && seg_len_hint <= 48) {
                    *name = FILT ? "range_scan_bitmap_kernel+filter" : "range_scan_bitmap_kernel";
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
            *name = CS > 0 ? (FILT ? "range_scan_kernel+filter" : "range_scan_kernel")
                           : (FILT ? "range_scan_kernel (run-time code size)+filter" : "range_scan_kernel (run-time code size)");
            hipLaunchKernelGGL(kern, grid, block, shm, s, t.codes, t.norm_codes, luts, t.norm_table, p.segs, p.lpos, p.hdr,
                               p.max_seg, nsplit, t.M, radius, slices, out, m...);
            return hipGetLastError();
        });
    });
}

} // namespace

hipError_t launch_range_count(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int nsplit,
                              int seg_len_hint, float radius, uint32_t *slices, unsigned long long *total,
                              const uint32_t *fmask, const char **kernel_name)
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
                             const uint32_t *fmask)
{
    if (p.nq == 0)
        return hipSuccess;
    const char *name = "";
    return range_launch<true>(s, t, luts, p, nsplit, seg_len_hint, radius, const_cast<uint32_t *>(bases),
                              RangeOut{t.ids, dist, reinterpret_cast<long long *>(labels)}, fmask, &name);
}

} // namespace ivfhnsw_gpu_impl
