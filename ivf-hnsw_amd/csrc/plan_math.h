// The arithmetic the kernels that BUILD a scan plan share (plan_ivf_kernel, ivf_tail_kernel, plan_grouping_kernel,
// plan_grouping4_kernel): the max_codes rules as functions of prefix sums of list sizes, the hash of the
// neighbour-centroid set, and the layout of the four-wave kernel's dynamic LDS.  One copy; the device steps are in
// plan_steps.h.  No HIP in here: tests/cpp/plan_math_tool.cpp checks it on the host against plain serial loops.
#pragma once

#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define IVFHNSW_PLAN_FN __host__ __device__ __forceinline__
#else
#define IVFHNSW_PLAN_FN inline
#endif

namespace ivfhnsw_gpu_impl {

// ---- the max_codes rules.  A query's probed lists in probe order have sizes n_i; incl_i = n_0 + .. + n_i and
// excl_i = incl_i - n_i.  The reference checks its budget AFTER scoring a list (IndexIVF_HNSW.cpp:290-292,
// Grouping.cpp:256-258, :350-352), so the first non-empty list is always scored.
//
// IVFADC: list i is scored iff it is non-empty and fewer than max_codes codes precede it (or none does).
IVFHNSW_PLAN_FN bool plan_budget_open(unsigned long long excl, unsigned long long max_codes)
{
    return excl < max_codes || excl == 0;
}
IVFHNSW_PLAN_FN bool plan_takes_list(unsigned long long n, unsigned long long excl, unsigned long long max_codes)
{
    return n != 0 && plan_budget_open(excl, max_codes);
}
// Grouping, pass 1: the last row (non-empty list) visited is the first whose inclusive sum reaches 2 * max_codes.
IVFHNSW_PLAN_FN bool plan_pass1_ends(unsigned long long incl, unsigned long long max_codes)
{
    return incl >= 2 * max_codes;
}
// Pass 2 (and the IVFADC scan): the last row visited is the first at which the codes scored reach max_codes.  Without
// pruning every code of a visited list is scored, so this is a rule on the inclusive sum of list sizes too.
IVFHNSW_PLAN_FN bool plan_pass2_ends(unsigned long long incl, unsigned long long max_codes)
{
    return incl >= max_codes;
}

// ---- the LDS hash set of a query's distinct neighbour centroids (plan_grouping4_kernel<true>): linear probing, at
// most GH_PROBES steps, after which the pair's row is gathered directly.
constexpr int GH_SLOTS = 2048;
constexpr int GH_PROBES = 48;
constexpr uint32_t GH_EMPTY = 0xffffffffu;

IVFHNSW_PLAN_FN uint32_t gh_hash(uint32_t id) { return (id * 2654435761u) >> 21; } // 11 bits

// ---- dynamic LDS of plan_grouping4_kernel, in 4-byte words from its start: the query float[d] at 0, a 64-float
// hand-back area per wavefront at `dist`, then one array of nprobe words per Plan4Row at row(a).  A row is a non-empty
// probed group, in probe order (at most nprobe of them); what wavefront 0's serial passes need of it is staged once, so
// that they read LDS instead of chains of dependent global loads.
enum Plan4Row { // probe index, centroid, list size, alpha, ||c||^2, first local code, coarse distance, active sub-groups
    kRowProbe, kRowCentroid, kRowSize, kRowAlpha, kRowNorm, kRowFirstCode, kRowCoarseDist, kRowActive, kPlan4Rows
};
struct Plan4Lds {
    uint32_t dist, rows, nprobe, words;
    IVFHNSW_PLAN_FN uint32_t row(int a) const { return rows + (uint32_t)a * nprobe; }
    IVFHNSW_PLAN_FN size_t bytes() const { return (size_t)words * 4; }
};
IVFHNSW_PLAN_FN Plan4Lds plan4_lds(int d, int nprobe)
{
    const uint32_t rows = (uint32_t)d + 4 * 64;
    return Plan4Lds{(uint32_t)d, rows, (uint32_t)nprobe, rows + kPlan4Rows * (uint32_t)nprobe};
}

} // namespace ivfhnsw_gpu_impl
