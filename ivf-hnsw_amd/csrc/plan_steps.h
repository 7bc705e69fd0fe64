// The steps the kernels that build a scan plan share, one copy each: the IVFADC plan of one chunk of 64
// probes (plan_ivf_kernel, plan_lut_kernel, ivf_tail_kernel), and for the Grouping plan (plan_grouping_kernel,
// plan_grouping4_kernel) the gather of neighbour-centroid distances by lane quads, the segments a chunk of sub-groups
// emits, the threshold sum, the hash-set probe and -- the parity contract -- the float formulas in the reference's
// order.  Control flow (which rows a wavefront takes, what is loaded a row ahead, the branch on a ballot, the stamps) is
// the kernels'.  The rules and layouts as plain arithmetic: plan_math.h.
#pragma once

#include "ivfhnsw_kernels.h"
#include "device_common.h"
#include "plan_math.h"

namespace ivfhnsw_gpu_impl {

// Where a query's plan stands: codes visited so far == scan position of the next one (wave-uniform), segments and codes
// emitted on this shard.
struct PlanCursor {
    unsigned long long ncode = 0;
    uint32_t ns = 0, nl = 0;
};

__device__ __forceinline__ void store_plan_hdr(PlanHdr *dst, uint32_t ns, uint32_t nl)
{
    PlanHdr h;
    h.nseg = ns;
    h.total = nl;
    *dst = h;
}

// ---------------------------------------------------------------------------------------------------------------------
// IVFADC (IndexIVF_HNSW.cpp:267-292)
// ---------------------------------------------------------------------------------------------------------------------
// cterm of a list: ||x - c||^2 - ||c||^2
__device__ __forceinline__ float ivf_cterm(float coarse_dist, float centroid_norm)
{
    return __fsub_rn(coarse_dist, centroid_norm);
}

// One wavefront, probes [base, base + 64) of a query, a lane per probe: list sizes in parallel, the max_codes prefix
// rule by a wave scan, a segment per scored list this shard owns.  qc / qd: the query's coarse ids and distances.
__device__ __forceinline__ void ivf_plan_chunk(PlanCursor &cur, const IvfTables &t, const uint32_t *__restrict__ qc,
                                               const float *__restrict__ qd, int base, int nprobe,
                                               unsigned long long max_codes, Seg *sq, uint32_t *lq, int lane)
{
    const int i = base + lane;
    uint32_t c = 0xffffffffu;
    if (i < nprobe)
        c = qc[i];
    const bool ok = c < t.nc; // padding slots (fewer than nprobe coarse results) hold 0xffffffff
    unsigned long long n = 0;
    if (ok)
        n = t.goff[c + 1] - t.goff[c];
    const unsigned long long incl = wave_incl_scan_u64(n, lane) + cur.ncode;
    const unsigned long long excl = incl - n;
    const bool take = plan_takes_list(n, excl, max_codes);
    const uint32_t lo_c = take ? t.loff[c] : kNotOwned;
    const bool owned = lo_c != kNotOwned;
    const unsigned long long om = __ballot(owned);
    const unsigned long long own_incl = wave_incl_scan_u64(owned ? n : 0ull, lane);
    if (owned) {
        const uint32_t r = cur.ns + (uint32_t)__popcll(om & ((1ull << lane) - 1ull));
        Seg sg;
        sg.start = lo_c;
        sg.len = (uint32_t)n;
        sg.vpos = (uint32_t)excl;
        sg.cterm = ivf_cterm(qd[i], t.centroid_norms[c]);
        sq[r] = sg;
        lq[r] = cur.nl + (uint32_t)(own_incl - n);
    }
    cur.ns += (uint32_t)__popcll(om);
    cur.nl += (uint32_t)__shfl(own_incl, 63, 64);
    // codes visited: everything up to and including the list that reached max_codes
    const unsigned long long stop = __ballot(take && plan_pass2_ends(incl, max_codes));
    const int last = stop ? __ffsll((long long)stop) - 1 : 63;
    cur.ncode = __shfl(incl, last, 64);
}

// ---------------------------------------------------------------------------------------------------------------------
// Grouping (IndexIVF_HNSW_Grouping.cpp:222-353)
// ---------------------------------------------------------------------------------------------------------------------
// The constants of a probed group: term1 = (1 - alpha) * x, x = the coarse distance in pass 1 (:251), the coarse distance
// less ||c||^2 (ivf_cterm) in pass 2 (:318).
struct GroupTerms {
    float alpha, oma, term1;
};
__device__ __forceinline__ GroupTerms group_terms(float alpha, float x)
{
    const float oma = __fsub_rn(1.0f, alpha);
    return GroupTerms{alpha, oma, __fmul_rn(oma, x)};
}
// pass-1 value of a sub-group (Grouping.cpp:251-252): inter = its inter-centroid distance, qn = ||x - y_N||^2
__device__ __forceinline__ float group_pass1_value(const GroupTerms &gt, float inter, float qn)
{
    const float a = __fmul_rn(gt.oma, inter);
    const float b = __fsub_rn(a, qn);
    return __fsub_rn(gt.term1, __fmul_rn(gt.alpha, b));
}
// cterm of a sub-group, term1 + term2 (Grouping.cpp:318): nn_norm = ||y_N||^2
__device__ __forceinline__ float group_cterm(const GroupTerms &gt, float qn, float nn_norm)
{
    const float term2 = __fmul_rn(gt.alpha, __fsub_rn(qn, nn_norm));
    return __fadd_rn(gt.term1, term2);
}

__device__ __forceinline__ void wave_lds_order()
{
    // LDS operations of one wavefront execute in order; this only stops hipcc from moving them across each other
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
}

// ||x - y_N||^2 for the lanes that ask (`am` = their ballot, taken by the kernel, which may branch on it), N = the
// lane's nn: a quad of lanes per row, 16 rows per pass, results handed back to the asking lane through s_dist[64].
// Returns the lane's distance; a lane that did not ask gets `held` back.  FOUR_WAVES: the four-wave kernel's pair of
// distance function and LDS ordering; the one-wavefront kernel keeps the pair it was written and measured with.
template <bool FOUR_WAVES>
__device__ __forceinline__ float gather_quads(bool ask, unsigned long long am, uint32_t nn, float held,
                                              const float *__restrict__ vectors, const float *s_q, int d, float *s_dist,
                                              int lane)
{
    const int na = __popcll(am);
    for (int base = 0; base < na; base += 16) {
        const int r = base + (lane >> 2);
        const int src = r < na ? nth_set_bit(am, r) : 0;
        const uint32_t nnq = (uint32_t)__shfl((int)nn, src, 64);
        float dq = 0.f;
        if (r < na)
            dq = FOUR_WAVES ? l2_ref_order_quad_batched(vectors + (size_t)nnq * d, s_q, d, lane & 3)
                            : l2_ref_order_quad(vectors + (size_t)nnq * d, s_q, d, lane & 3);
        if (r < na && (lane & 3) == 0)
            s_dist[src] = dq;
    }
    FOUR_WAVES ? wave_lds_order() : __syncthreads();
    if (ask)
        held = s_dist[lane];
    FOUR_WAVES ? wave_lds_order() : __syncthreads();
    return held;
}

// threshold += the pass-1 values of a chunk's active sub-groups, in sub-group order (Grouping.cpp:253)
__device__ __forceinline__ void threshold_add_active(float &threshold, unsigned long long &nsubgroups, bool active, float v)
{
    unsigned long long m = __ballot(active);
    nsubgroups += __popcll(m);
    while (m) {
        const int j = __ffsll((long long)m) - 1;
        m &= m - 1;
        threshold = __fadd_rn(threshold, __shfl(v, j, 64));
    }
}

// The segments of one chunk of 64 sub-groups of a list (a lane per sub-group, sz = its size, 0 beyond nsubc): one per
// scanned sub-group if this shard owns the list, in sub-group order.  lo_c = the list's first local code, list_off = the
// codes of the list before this chunk.  Returns the chunk's codes, scanned or not.
__device__ __forceinline__ uint32_t emit_segments(PlanCursor &cur, bool scanned, uint32_t sz, float cterm, uint32_t lo_c,
                                                  uint32_t list_off, Seg *sq, uint32_t *lq, int lane)
{
    const bool owned = lo_c != kNotOwned;
    const uint32_t in_sz = wave_incl_scan(sz, lane);
    const uint32_t in_sc = wave_incl_scan(scanned ? sz : 0u, lane);
    const unsigned long long m = __ballot(scanned);
    const uint32_t rank_sc = __popcll(m & ((1ull << lane) - 1ull));
    if (scanned && owned) {
        Seg sg;
        sg.start = lo_c + list_off + (in_sz - sz);
        sg.len = sz;
        sg.vpos = (uint32_t)cur.ncode + (in_sc - sz);
        sg.cterm = cterm;
        sq[cur.ns + rank_sc] = sg;
        lq[cur.ns + rank_sc] = cur.nl + (in_sc - sz);
    }
    const uint32_t tot_sz = __shfl(in_sz, 63, 64), tot_sc = __shfl(in_sc, 63, 64);
    cur.ncode += tot_sc;
    if (owned) {
        cur.ns += (uint32_t)__popcll(m);
        cur.nl += tot_sc;
    }
    return tot_sz;
}

// The slot of centroid id nn in the hash set, or -1: INSERT enters it where it is missing (-1: no slot within GH_PROBES
// steps); otherwise -1 means it was never entered.
template <bool INSERT> __device__ __forceinline__ int gh_find(uint32_t *h_key, uint32_t nn)
{
    uint32_t slot = gh_hash(nn);
    int found = -1;
    // pinned to what the two loops compiled to when each was written out in its kernel phase (left alone, the shared
    // form is unrolled 48 times: 1200 instructions more)
    constexpr int kUnroll = INSERT ? 8 : 1;
#pragma unroll kUnroll
    for (int pr = 0; pr < GH_PROBES; pr++) {
        uint32_t kk;
        if constexpr (INSERT)
            kk = atomicCAS(&h_key[slot], GH_EMPTY, nn);
        else
            kk = h_key[slot];
        if (kk == GH_EMPTY || kk == nn) {
            if (INSERT || kk == nn)
                found = (int)slot;
            break;
        }
        slot = (slot + 1) & (GH_SLOTS - 1);
    }
    return found;
}

} // namespace ivfhnsw_gpu_impl
