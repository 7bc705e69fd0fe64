// The steps the ADC scan kernels share, one copy each: how a staged plan chunk is walked, how a table and
// a plan chunk reach LDS, and -- the parity contract -- how a code's distance and its key are formed.  A kernel that
// scores a code calls adc_distance / adc_key; what it does with the result (minimum, sort buffer, heap, hit list) is its
// own.  Index arithmetic: scan_plan_math.h.
#pragma once

#include "ivfhnsw_kernels.h"
#include "device_common.h"
#include "scan_plan_math.h"

namespace ivfhnsw_gpu_impl {

// dist = (cterm + norm) - 2 * sum (IndexIVF_HNSW.cpp:286), every step an explicit round-to-nearest intrinsic.  (Callers
// take the table sum into a local first: written as the argument it is issued behind the norm read, one VGPR more.)
__device__ __forceinline__ float adc_distance(float cterm, float norm, float sum)
{
    const float tt = __fadd_rn(cterm, norm);
    return __fsub_rn(tt, __fmul_rn(2.0f, sum));
}
// the distance as results carry it: -0 folded into +0, so equal distances have equal bits (and equal keys)
__device__ __forceinline__ float adc_value(float dist) { return __fadd_rn(dist, 0.0f); }
// packed (distance, scan position): unsigned order = the reference's strict-'<' first-wins order
__device__ __forceinline__ unsigned long long adc_key(float dist, uint32_t vpos)
{
    return ((unsigned long long)f32_orderable(adc_value(dist)) << 32) | vpos;
}

// The ADC sum of one code from the query's table in LDS, m = 0..CS-1 in order (IndexIVF_HNSW.cpp:802-814), the table
// addressed by byte offset (code_sum, device_common.h, is the indexed form; the sum is the same).  The run-time form's
// sum was taken while the code was read (code_fetch).
template <int CS> __device__ __forceinline__ float code_sum_lds(const float *s_lut, const CodeRegs<CS> &r)
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

// A row's norm code and, under a label filter (device_common.h filter_mask), the 32-bit mask word that holds the row's
// bit: loaded side by side, so both waits fall together.
// KIND: filter_kind (device_common.h).  Under filter slots (2) a query without a plane (FilterFill: keep = 0) reads word 0
// whatever the row, so that no branch stands here; nothing is done to the loaded word before filter_pass, because a use
// of it here makes the compiler wait for each unrolled step's loads before it issues the next step's.  Under row tags (3,
// DESIGN.md 3.21) the word is the row's tag and a handle without tags (keep = 0) reads element 0 the same way.  Under row
// values (4) it is the row's uint32, read the same way.  Under tag AND value (5) a row
// brings both, so the word a kernel carries from its load loop to filter_pass is a pair there (FilterWord) and a bare
// uint32_t in every other kind; the values come from fmask, the tags from fill.rtags, each masked by its own keep.
template <int KIND>
__device__ __forceinline__ void load_norm_filter(const uint8_t *norm_codes, const uint32_t *fmask, uint32_t row, uint32_t &nb,
                                                 FilterWord<KIND> &fw, [[maybe_unused]] const FilterFill &fill = FilterFill())
{
    nb = norm_codes[row];
    if constexpr (KIND == 1)
        fw = fmask[row >> 5];
    if constexpr (KIND == 2)
        fw = fmask[(row >> 5) & fill.keep];
    if constexpr (KIND == 3) // the row's 16-bit tag, zero-extended: the 64 lanes of a wavefront read 128 contiguous bytes
        fw = reinterpret_cast<const uint16_t *>(fmask)[row & fill.keep];
    if constexpr (KIND == 4) // the row's value: one dword, the 64 lanes of a wavefront read 256 contiguous bytes
        fw = fmask[value_index(row, fill.keep)];
    if constexpr (KIND == 5) { // both: 128 + 256 contiguous bytes per wavefront, issued side by side
        fw.t = fill.rtags[tag_index(row, fill.tkeep)];
        fw.v = fmask[value_index(row, fill.keep)];
    }
}
// fb = row & 31: the row's bit in that word
__device__ __forceinline__ bool filter_pass(uint32_t fw, uint32_t fb) { return (fw >> fb) & 1u; }
// ... under filter slots through the query's two scalars: the plane's word, all ones (NONE) or zero (no such slot)
template <int KIND> __device__ __forceinline__ bool filter_pass(uint32_t fw, uint32_t fb, [[maybe_unused]] const FilterFill &fill)
{
    if constexpr (KIND == 2)
        fw = (fw & fill.keep) | fill.all;
    if constexpr (KIND == 3) // a tag per row: equal to the query's scalar, or the query is untagged (wave-uniform); no branch
        return (fw == fill.all) | (fill.all == 0xffffu);
    if constexpr (KIND == 4) // a value per row: inside the query's interval (value_math.h); no branch
        return value_pass(fw, fill.keep, fill.all, fill.span, fill.live);
    return (fw >> fb) & 1u;
}
// ... and under tag AND value (5) with the row's pair of words: the AND of the two rules above (tag_value_math.h); no branch
template <int KIND> __device__ __forceinline__ bool filter_pass(const TagValueWord &fw, uint32_t, const FilterFill &fill)
{
    static_assert(KIND == 5, "a pair of words is the sixth form's");
    return tag_value_pass(fw.t, fw.v, fill.tag, fill.keep, fill.all, fill.span, fill.live);
}

// The table of query q into LDS, global -> LDS directly (global_load_lds_dwordx4: wave-uniform LDS base + lane * 16): the
// table never passes through VGPRs, and a ds_write_b128 costs the LDS pipe 13 cycles where the DMA's write costs 4 -- the
// scan is bound by that pipe.  The caller's next __syncthreads waits for it.
template <int THREADS>
__device__ __forceinline__ void stage_table_dma(const float *luts, int q, int csz, float *s_lut, int tid)
{
    const float4 *src = reinterpret_cast<const float4 *>(luts + (size_t)q * csz * 256);
    const int lane = tid & 63;
    for (int i = tid; i < csz * 64; i += THREADS)
        __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + i),
                                         (__attribute__((address_space(3))) void *)(reinterpret_cast<float4 *>(s_lut) + (i - lane)),
                                         16, 0, 0);
}

// Segments [cs, cs + cn) of a query's plan (sq, lq) into s_seg / s_lpos, and the chunk's end ch (plan_chunk_end) into
// s_lpos[cn].  Between two barriers of the caller's.
template <int THREADS>
__device__ __forceinline__ void stage_plan_chunk(const Seg *sq, const uint32_t *lq, uint32_t cs, uint32_t cn, uint32_t ch,
                                                 Seg *s_seg, uint32_t *s_lpos, int tid)
{
    for (uint32_t i = tid; i < cn; i += THREADS) {
        s_seg[i] = sq[cs + i];
        s_lpos[i] = lq[cs + i];
    }
    if (tid == 0)
        s_lpos[cn] = ch;
}

// The segment a lane is inside, in registers: positions only grow, so the LDS plan is consulted again only when a
// position runs past the segment's end.  One cursor per staged chunk.
struct SegCursor {
    uint32_t s = 0, seg_lo = 0, seg_hi = 0, seg_start = 0, seg_vpos = 0;
    float seg_ct = 0.f;

    // move to position p (Policy: scan_plan_math.h)
    template <class Policy>
    __device__ __forceinline__ void seek(uint32_t p, const uint32_t *s_lpos, const Seg *s_seg, uint32_t cn)
    {
        if (p >= seg_hi) {
            s = Policy::seek(s_lpos, s, cn, p);
            const Seg sg = s_seg[s];
            seg_lo = s_lpos[s];
            seg_hi = seg_lo + sg.len;
            seg_start = sg.start;
            seg_vpos = sg.vpos;
            seg_ct = sg.cterm;
        }
    }
};

// One chunk of the bitmap form (scan_plan_math.h bitmap_extent) staged in the kernel's own LDS arrays: the segments, a
// bit per position set where a segment starts, and the starts before every 64-position word.  A wavefront's 64 positions
// share a word, so the segment of a position is one broadcast LDS read and two v_mbcnt.
struct BitmapChunk {
    uint32_t cn, ch;
    bool single;
    const unsigned long long *s_mask;
    const uint32_t *s_pref;

    // the bitmap word of chunk-relative position r (wave-uniform: a wavefront's positions start at a multiple of 64)
    static __device__ __forceinline__ uint32_t word_of(uint32_t r) { return __builtin_amdgcn_readfirstlane(r >> 6); }
    // the chunk segment of the position at bit `lane` of word wi
    __device__ __forceinline__ uint32_t segment_of(uint32_t wi, int lane) const
    {
        if (single)
            return 0;
        const unsigned long long mw = s_mask[wi];
        const uint32_t below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mw >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mw, 0u));
        return bitmap_segment(s_pref[wi], mw, below, lane);
    }
};

// Stage the chunk that starts at segment cs.  All THREADS threads call it; it opens with the barrier that ends the
// previous chunk's use of the arrays (and, the first time, completes the table staging).
template <int THREADS>
__device__ __forceinline__ BitmapChunk stage_bitmap_chunk(const Seg *sq, const uint32_t *lq,
                                                          uint32_t cs, uint32_t nseg, uint32_t total, Seg *s_seg,
                                                          uint32_t *s_lpos, unsigned long long *s_mask, uint32_t *s_pref,
                                                          uint32_t *s_wtot, int tid)
{
    static_assert(THREADS >= kBmSpanWords && kBmSpanWords <= 128, "one thread per word; waves 0 and 1 scan, two totals");
    const int lane = tid & 63, wave = tid >> 6;
    const uint32_t cl = lq[cs];
    const BitmapExtent e = bitmap_extent(lq, cs, nseg, total);
    __syncthreads();
    for (uint32_t i = tid; i < e.cn; i += THREADS) {
        s_seg[i] = sq[cs + i];
        s_lpos[i] = lq[cs + i];
    }
    if (tid < (int)e.nwords)
        s_mask[tid] = 0ull;
    __syncthreads();
    if (!e.single) {
        uint32_t *m32 = reinterpret_cast<uint32_t *>(s_mask);
        for (uint32_t i = tid; i < e.cn; i += THREADS) {
            const uint32_t r = s_lpos[i] - cl;
            atomicOr(&m32[r >> 5], 1u << (r & 31));
        }
        __syncthreads();
        const uint32_t cnt = tid < (int)e.nwords ? (uint32_t)__popcll(s_mask[tid]) : 0u;
        const uint32_t inc = wave_incl_scan(cnt, lane);
        if (lane == 63)
            s_wtot[wave] = inc;
        __syncthreads();
        if (tid < (int)e.nwords)
            s_pref[tid] = (wave ? s_wtot[0] : 0u) + inc - cnt;
        __syncthreads();
    }
    return BitmapChunk{e.cn, e.ch, e.single, s_mask, s_pref};
}

} // namespace ivfhnsw_gpu_impl
