// Which instantiation of the throughput walk (kernels_hnsw.hip) a launch takes, and how much dynamic LDS it asks for:
// the whole rule, from the graph, efSearch and the environment's knobs to the kernel's template arguments.  A wrong
// choice here computes nothing wrong (every form is exact) and only costs time, so the rule is plain host C++ with no
// HIP in it, and tests/cpp/walk_form_tool.cpp checks it on the host.  launch_coarse: with_walk_form(walk_form_for(...), f).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <type_traits>

namespace ivfhnsw_gpu_impl {

constexpr int kTailCap = 64; // entries of the LDS tail (walk_set.h): evicted candidates that tie with the lower bound

// What the environment says, read once per process (walk_knobs, kernels_hnsw.hip).
struct WalkKnobs {
    bool force_bitmap = false; // IVFHNSW_WALK_VIS=bitmap: global visited bitmaps, no LDS set (A/B runs)
    int force_tagw = 0;        // IVFHNSW_WALK_TAGW=10|12|16: a wider tag than the graph needs (tests: small graphs reach every form)
    bool shape_on = true;      // IVFHNSW_WALK_SHAPE=0: always the generic instantiation (A/B runs)
    bool stamps = false;       // IVFHNSW_WALK_STAMPS=1: the diagnostic build, where one exists
};

// The facts of a GraphTables that the rule reads.
struct WalkGraph {
    uint32_t n;
    int d, maxM, nb_rows;
    bool qrows, nbrows, links_unique, merge_admissions; // the byte rows / the neighbour rows exist; its two flags
};

// Everything a launch needs to know: hnsw_walk_kernel's template arguments, the bucket count and the dynamic LDS.
struct WalkForm {
    int nch;      // 64-entry registers of the result set: 1, 2, 3, 4, 8 or 16
    int tagw;     // bits per tag of the LDS visited set: 8, 10, 12, 16; 0 = global bitmaps only
    int nbuckets; // its buckets (walk_vis_buckets; 0 without the set): not an argument, it follows from tagw
    int fmode;    // rejection filter: 0 off, 1 gather from qrows, 2 neighbour rows, 3 neighbour rows with late visited entry
    int d, maxM;  // the shape compiled in: 128 or 96 / 32; 0 / 0 = the generic form, which reads the shape at run time
    bool merge;   // shaped forms: the graph's merge_admissions; the generic form reads that at run time and has `true` here
    bool stamps;  // the diagnostic build with per-segment cycle sums
    size_t lds_bytes;
};

// Buckets of the LDS visited set.  The kernel is built for 4 waves per SIMD, 16 per CU sharing 160 KB of LDS: 1008
// buckets = 7.9 KB (with query, planes, tail and merge buffer 9.8 KB per wave at efSearch 80: sixteen waves fill 157 of
// the 160 KB).  10-bit tags (six per bucket) exist for graphs of about a million nodes -- the reference's 993 127
// centroids, the 2^20 of the 8-GPU bench: with 12-bit tags (five per bucket) 896 buckets ran 56 % full and every
// expansion paid a global atomic for an overflowing neighbour.  1040 buckets x 6 = 6240 slots, 8320 bytes.
constexpr int walk_vis_buckets(int tagw) { return tagw == 10 ? 1040 : 1008; }

// IVFHNSW_WALK_LATE_VISIT unset (capi_upload.cpp): late visited entry where ids need more than 8 tag bits
inline bool walk_late_visit_default(size_t n) { return n > 255u * (size_t)walk_vis_buckets(8); }

// 64-entry registers of the result set, in classes (3: efSearch 129..192 -- the reference's DEEP1B presets use 130)
inline int walk_nch_for(int ef) { return ef <= 64 ? 1 : ef <= 256 ? (ef + 63) / 64 : ef <= 512 ? 8 : 16; }

// How many wavefront slots the walk keeps resident for a given ef (sizes the visited bitmaps).  Exactly the wavefronts
// that can be resident (256 CUs x 4 SIMDs x 4 waves per SIMD, 3 where the result set takes 16 registers; the kernel's
// registers allow no more): blocks beyond that only start when a slot frees up, find the queue empty and cost their
// prologue -- 1.205 vs 1.189 ms per 10 k queries with 8192 instead of 4096 blocks.
inline int coarse_slots_for(int ef) { return 256 * 4 * (walk_nch_for(ef) <= 8 ? 4 : 3); }

// dynamic LDS: float query[d] (twice for the gather form) | four byte planes of the query | u64 tail[kTailCap], which
// doubles as the merge buffer of a pass's admissions (ef + 8 entries, ef <= 256) | u64 visited set[buckets]
inline size_t walk_lds_bytes(int d, bool gather, int ef, int tagw)
{
    const int merge_extra = (ef <= 256 && ef + 8 > kTailCap) ? ef + 8 - kTailCap : 0;
    return (size_t)(d + (gather ? d : 0)) * sizeof(float) + 512 + (size_t)(kTailCap + merge_extra) * sizeof(uint64_t) +
           (tagw ? (size_t)walk_vis_buckets(tagw) * sizeof(uint64_t) : 0);
}

inline WalkForm walk_form_for(const WalkGraph &g, int ef, const WalkKnobs &k)
{
    WalkForm f = {};
    f.nch = walk_nch_for(ef);
    // the tag (id / buckets + 1) must fit: 8 bits up to 255 * buckets nodes, ..., 16 bits at most
    const uint32_t nbk = (uint32_t)walk_vis_buckets(8);
    f.tagw = k.force_bitmap ? 0 : g.n <= 255u * nbk ? 8 : g.n <= 4095u * nbk ? 12 : g.n <= 65535u * nbk ? 16 : 0;
    if (f.tagw && k.force_tagw > f.tagw)
        f.tagw = k.force_tagw;
    if ((f.tagw == 12 || f.tagw == 10) && g.n <= 1023u * (uint32_t)walk_vis_buckets(10) && k.force_tagw != 12)
        f.tagw = 10;
    f.nbuckets = f.tagw ? walk_vis_buckets(f.tagw) : 0;
    f.fmode = g.nbrows ? (g.links_unique && f.tagw ? 3 : 2) : g.qrows ? 1 : 0;
    f.lds_bytes = walk_lds_bytes(g.d, f.fmode == 1, ef, f.tagw);
    // The shaped forms exist for the neighbour-row filter (fmode 2 and 3) with the LDS visited set, result sets of up to
    // 128 entries, 32 links per node in one 32-row record, and the two row lengths whose query share lives in registers
    // (128: SIFT, 96: DEEP).  Everything else is the generic form.
    if (k.shape_on && f.fmode >= 2 && f.tagw != 0 && ef >= 1 && f.nch <= 2 && g.maxM == 32 && g.nb_rows == 32 &&
        (g.d == 128 || g.d == 96)) {
        f.d = g.d;
        f.maxM = 32;
    }
    // The diagnostic build exists for the two forms the bench's graphs take at ef 80 / 100 (2^17 nodes; about a million),
    // the second also with the shape compiled in (d 128, merge), so that the stamps describe the code that is timed.
    f.stamps = k.stamps && f.nch == 2 && ((f.tagw == 8 && f.fmode == 2) || (f.tagw == 10 && f.fmode == 3));
    if (f.stamps && !(f.tagw == 10 && f.d == 128 && g.merge_admissions))
        f.d = f.maxM = 0;
    f.merge = f.d == 0 || g.merge_admissions;
    return f;
}

// The redo launch (launch_coarse_redo): the plainest form -- no filter, global bitmaps -- of the same nch class.
inline WalkForm walk_redo_form(const WalkGraph &g, int ef)
{
    return {walk_nch_for(ef), 0, 0, 0, 0, 0, true, false, walk_lds_bytes(g.d, false, ef, 0)};
}

template <int N> using walk_int = std::integral_constant<int, N>;

// f(walk_int<V>()) for the V of Vs that equals v; false when there is none, else what f returns
template <class F> bool walk_pick(int, F &&) { return false; }
template <int V, int... Vs, class F> bool walk_pick(int v, F &&f)
{
    if (v == V)
        return f(walk_int<V>());
    return walk_pick<Vs...>(v, f);
}

// f(walk_int<nch>()) for an nch class up to MAXN; false for anything else
template <int MAXN = 16, class F> bool with_walk_nch(int nch, F &&f)
{
    return walk_pick<1, 2, 3, 4, 8, 16>(nch, [&](auto n) {
        if constexpr (decltype(n)::value <= MAXN)
            f(n);
        return decltype(n)::value <= MAXN;
    });
}

// f(nch, tagw, fmode, stamps, d, maxM, merge) with the form's values as integral constants; false, and no call, for a form
// without an instantiation.  This is the list of the fast forms that exist: what f does is compiled once for each.
template <class F> bool with_walk_form(const WalkForm &w, F &&f)
{
    using no = std::false_type;
    using yes = std::true_type;
    if (w.nbuckets != (w.tagw ? walk_vis_buckets(w.tagw) : 0) || w.maxM != (w.d ? 32 : 0))
        return false;
    if (w.stamps) { // the three diagnostic builds
        const bool small = w.tagw == 8 && w.fmode == 2 && w.d == 0, big = w.tagw == 10 && w.fmode == 3 && (w.d == 0 || w.d == 128);
        if (w.nch != 2 || !w.merge || !(small || big))
            return false;
        if (small)
            f(walk_int<2>(), walk_int<8>(), walk_int<2>(), yes(), walk_int<0>(), walk_int<0>(), yes());
        else if (w.d == 0)
            f(walk_int<2>(), walk_int<10>(), walk_int<3>(), yes(), walk_int<0>(), walk_int<0>(), yes());
        else
            f(walk_int<2>(), walk_int<10>(), walk_int<3>(), yes(), walk_int<128>(), walk_int<32>(), yes());
        return true;
    }
    if (w.d != 0) // shaped: nch 1 and 2, LDS set, neighbour rows, d 128 / 96, either way of admitting
        return walk_pick<1, 2>(w.nch, [&](auto n) {
            return walk_pick<8, 10, 12, 16>(w.tagw, [&](auto t) {
                return walk_pick<2, 3>(w.fmode, [&](auto fm) {
                    return walk_pick<128, 96>(w.d, [&](auto d) {
                        w.merge ? f(n, t, fm, no(), d, walk_int<32>(), yes()) : f(n, t, fm, no(), d, walk_int<32>(), no());
                        return true;
                    });
                });
            });
        });
    if (!w.merge)
        return false;
    // generic: every nch class, every tag width, every filter form -- but late visited entry needs the LDS set
    return walk_pick<1, 2, 3, 4, 8, 16>(w.nch, [&](auto n) {
        return walk_pick<0, 8, 10, 12, 16>(w.tagw, [&](auto t) {
            return walk_pick<0, 1, 2, 3>(w.fmode, [&](auto fm) {
                constexpr bool exists = !(decltype(fm)::value == 3 && decltype(t)::value == 0);
                if constexpr (exists)
                    f(n, t, fm, no(), walk_int<0>(), walk_int<0>(), yes());
                return exists;
            });
        });
    });
}

} // namespace ivfhnsw_gpu_impl
