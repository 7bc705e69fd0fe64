// Device-side data layout and kernel launchers of the gfx950 IVFADC search path.
// Host code (capi_*.cpp) sees only the launch_* functions; kernels live in kernels_*.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <mutex>
#include <stdint.h>

#include "scan_dispatch.h"
#include "sweep_plan_math.h"
#include "update_math.h"
#include "walk_form.h"

namespace ivfhnsw_gpu_impl {

// hipFuncAttributeMaxDynamicSharedMemorySize is a property of (kernel, DEVICE): a process that drives several GPUs
// (the bundled classes with IVFHNSW_SHARDS=N, one host thread per shard) must raise it on each of them, and the
// bookkeeping of "already raised to ..." must be per device and safe against the shard threads.
struct DynLdsState {
    std::mutex m;
    size_t raised[64] = {};
};
inline hipError_t raise_dyn_lds(const void *kern, size_t bytes, DynLdsState &st)
{
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess)
        return e;
    if (dev < 0 || dev >= 64)
        return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    std::lock_guard<std::mutex> lk(st.m);
    if (bytes > st.raised[dev]) {
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
        if (e != hipSuccess)
            return e;
        st.raised[dev] = bytes;
    }
    return hipSuccess;
}
// what a launcher calls before a launch with `bytes` of dynamic LDS: every kernel KERN has a state of its own
template <auto KERN> hipError_t dyn_lds(size_t bytes)
{
    static DynLdsState st;
    return raise_dyn_lds((const void *)KERN, bytes, st);
}
// The dynamic LDS of a scan kernel KERN of code size CS: none for a compiled size, whose table is static LDS; for the
// run-time form (CS == 0) M KB, raised here, and hipErrorInvalidValue for an M it cannot take.
template <int CS, auto KERN> hipError_t scan_table_lds(int M, size_t *bytes)
{
    *bytes = 0;
    if constexpr (CS == 0) {
        if (!runtime_code_size_ok(M))
            return hipErrorInvalidValue;
        *bytes = (size_t)M * 1024;
        return dyn_lds<KERN>(*bytes);
    }
    return hipSuccess;
}

// One scored (sub)list of one query: the unit of the scan plan.
// start  : index of the first code inside this shard's flat code array
// len    : number of codes
// vpos   : position of the first code in the query's global scan order (tie-break, and label lookup)
// cterm  : the per-list constant of the distance: term1 (IndexIVF_HNSW.cpp:277) or term1+term2
//          (IndexIVF_HNSW_Grouping.cpp:290,318)
struct __attribute__((aligned(16))) Seg {
    uint32_t start;
    uint32_t len;
    uint32_t vpos;
    float cterm;
};

// Per-query plan header: nseg segments owned by this shard, `total` codes in them.
struct __attribute__((aligned(8))) PlanHdr {
    uint32_t nseg;
    uint32_t total;
};

// The scan plan of one batch as the launchers take it: segs / lpos [nq][max_seg] (lpos: a segment's first position in the
// query's flat array of owned codes), hdr [nq].  The launchers unpack it into their kernels' arguments; one that does not
// read lpos ignores it.
struct PlanView {
    Seg *segs;
    uint32_t *lpos;
    PlanHdr *hdr;
    int max_seg;
    int nq;
};

// The arrays of the resident lists that an in-place update fills beside the handle's (ListArrays::view, capi_internal.h):
// goff [nc + 1], loff [nc], and n_local rows of codes / ncodes / ids.
struct NewLists {
    uint64_t *goff;
    uint32_t *loff;
    uint8_t *codes, *ncodes;
    uint32_t *ids;
    uint64_t n_local;
};

// Packed result key: (orderable(dist) << 32) | vpos.  Unsigned order of the key is the order of
// (dist, scan position): strict '<' of IndexIVF_HNSW.cpp:285 == "smallest key wins".
constexpr uint32_t kOrdFltMax = 0x7f7fffffu | 0x80000000u; // orderable(FLT_MAX)
constexpr uint64_t kKeyInit = (uint64_t)kOrdFltMax << 32;  // accept iff key < kKeyInit
constexpr uint64_t kSignFlip = 0x8000000000000000ull;      // keys leave the library as signed-orderable int64

constexpr uint32_t kNotOwned = 0xffffffffu;

struct IvfTables {
    int d, M, dsub;             // M == code_size
    uint32_t nc;
    const uint64_t *goff;       // [nc+1] global list offsets
    const uint32_t *loff;       // [nc] first local code of list c; kNotOwned when the list lives on another shard
    const float *centroid_norms;
    const float *pq_centroids;  // [M][256][dsub]
    const float *norm_table;    // [256]
    const float *opq_At;        // [d][d] TRANSPOSED: At[k*d+i] = A[i][k], or null
    const uint8_t *codes;
    const uint8_t *norm_codes;
    const uint32_t *ids;
    uint32_t shard_rank, shard_world;
};

struct GroupTables {
    int nsubc;
    const float *alphas;
    const uint32_t *nn_idx;
    const uint32_t *sub_sizes;
    const float *inter_dists;
    int dedupe; // the plan evaluates every distinct neighbour centroid of a query once (kernels_grouping.hip DEDUPE): set at
                // upload when the neighbour lists of nearby groups overlap enough to pay for the hash set
};

struct GraphTables {
    uint32_t n;
    int d, maxM;
    uint32_t enterpoint;
    const uint8_t *counts;
    const uint32_t *links;   // [n][maxM]
    const float *vectors;    // [n][d]
    // Exact rejection filter of the walk (DESIGN.md "coarse walk"): every row once more as d bytes,
    // x ~ q_lo + q_step * byte, with q_errc >= max_row ||x - (q_lo + q_step*byte)|| / q_step.  NULL = filter off.
    const uint8_t *qrows;    // [n][d]
    float q_lo, q_step, q_errc;
    float q_errunit;         // q_errc / 511 rounded up: what one step of a row's error code is worth (walk_bound.h)
    // The same bytes once more, laid out for the walk (d <= 128): node i carries the byte rows of its own
    // neighbours, [n][nb_rows][128] with nb_rows = maxM rounded up to 32, zero padded.  One contiguous
    // nb_rows*128-byte read per expansion, issued together with the link list.  NULL = gather from qrows.
    const uint8_t *nbrows;
    // [n][nb_rows] sum of bytes^2 of every neighbour row (the filter's ||c||^2 term, 23 bits), and above it the row's own
    // error ||x - (q_lo + q_step*byte)|| / q_step in steps of q_errunit, rounded up (9 bits)
    const uint32_t *nbnorms;
    const uint32_t *links_c; // [n][maxM] id | (link count of id) << 24; goes with nbrows: the walk's keys carry the count
    int nb_rows;
    // Latency form of the walk (kernels_hnsw_lat.hip): node i carries the FLOAT rows of its own neighbours,
    // per node 32 rows of d floats (zero beyond the link count) and a 256-byte trailer with its links and link count;
    // NULL until ivfhnsw_gpu_prepare_latency builds it.
    const float *fat;
    int visited_clean;    // walk (set by its launcher): the global visited bitmaps are zero on entry and left zero
    // walk: insert a pass's admitted rows in one step (A/B knob IVFHNSW_WALK_MERGE=0); the generic form reads it, the
    // shaped forms are picked by it (hnsw_walk_kernel's MERGE)
    int merge_admissions;
    int links_unique;     // no id twice in a link list: survivors of the filter may enter the visited set late
};

// y[q][i] = fmaf chain over k of A[i][k] * x[q][k]  (IndexIVF_HNSW.cpp:240)
hipError_t launch_opq(hipStream_t s, const float *At, const float *x, float *y, int nq, int d);
// tab[q][m][c] = <x_m, centroid[m][c]>  (IndexIVF_HNSW.cpp:262)
// hdr (optional): queries whose plan is empty on this shard get no table
hipError_t launch_lut(hipStream_t s, const IvfTables &t, const float *xq, float *luts, int nq, const PlanHdr *hdr = nullptr);
// probe order + max_codes rule (IndexIVF_HNSW.cpp:267-292); also resets keys[nq*k] to kKeyInit
hipError_t launch_plan_ivf(hipStream_t s, const IvfTables &t, const uint32_t *coarse_ids, const float *coarse_dists,
                           int nprobe, uint64_t max_codes, const PlanView &p, uint64_t *keys, int k);
// plan_ivf + lut in one launch (one GPU; hipErrorInvalidValue for a dsub without an instantiation)
hipError_t launch_plan_lut(hipStream_t s, const IvfTables &t, const float *xq, const uint32_t *coarse_ids,
                           const float *coarse_dists, int nprobe, uint64_t max_codes, const PlanView &p, uint64_t *keys,
                           int k, float *luts);
// Grouping: sub-centroid distances, pruning threshold, pass-2 plan (IndexIVF_HNSW_Grouping.cpp:222-353)
hipError_t launch_plan_grouping(hipStream_t s, const IvfTables &t, const GroupTables &g, const GraphTables &gr,
                                const float *xq, const uint32_t *coarse_ids, const float *coarse_dists, int nprobe,
                                uint64_t max_codes, int do_pruning, const PlanView &p, uint64_t *keys, int k,
                                float *qsd_scratch);
// What launch_scan writes besides the keys, each part optional.
struct ScanOut {
    // k > 1: the candidate stream of the heap-order replay, stream_cap entries per query
    uint64_t *stream = nullptr;
    uint32_t *stream_len = nullptr;
    uint32_t stream_cap = 0;
    // k = 1: the scan resolves the winner's label itself where one workgroup sees the whole query
    float *sel_dist = nullptr;
    int64_t *sel_labels = nullptr;
};
// the ADC loop (IndexIVF_HNSW.cpp:282-289 / IndexIVF_HNSW_Grouping.cpp:321-333)
// seg_len_hint: expected codes per plan segment (0 = unknown), picks the scan form
// fmask (ScanFilter, scan_dispatch.h): a mask = the filtered form of the chosen kernel, bit r = local row r passes
// (launch_filter_mark); filter slots = its per-query form, a plane per slot and a slot byte per query
// *did_select: the scan wrote out.sel_dist / sel_labels (else launch_select has to run); *kernel_name: the form that ran,
// "" when nothing was launched; either may be null
hipError_t launch_scan(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int k, int nsplit,
                       uint64_t *keys, int seg_len_hint, const ScanFilter &fmask, const ScanOut &out, bool *did_select,
                       const char **kernel_name);
// table + scan pipelined over queries, for list shards (kernels_scan3.hip)
bool scan_pipe_supported(const IvfTables &t, int max_seg, int nq, int nsplit, bool has_codes, bool forced = false);
hipError_t launch_scan_pipe(hipStream_t s, const IvfTables &t, const float *xq, const PlanView &p, uint64_t *keys);
// plan + table + scan + select of a small IVFADC batch in one launch (kernels_tail.hip); keys_inv [nq] and done [nq] zeroed
bool ivf_tail_supported(const IvfTables &t, int nprobe, int k);
hipError_t launch_ivf_tail(hipStream_t s, const IvfTables &t, const float *xq, const uint32_t *cid, const float *cd,
                           int nq, int nprobe, uint64_t max_codes, int nsplit, uint64_t *keys_inv, uint32_t *done,
                           PlanHdr *hdr, float *dist, int64_t *labels, const uint32_t *status_word, uint32_t *status_out);
// k > 1 in faiss heap-array order: sequential replay of the top-k kernel's candidate stream
hipError_t launch_heap_replay(hipStream_t s, const IvfTables &t, const PlanView &p, const uint64_t *stream,
                              const uint32_t *stream_len, uint32_t stream_cap, int k, float *dist, int64_t *labels,
                              uint32_t *status,
                              int64_t *out_keys = nullptr, // non-null: the heap array as signed keys, no labels (sharded)
                              // non-null (labels path only): a query whose stream overflowed is appended to redo_list
                              // (redo_hdr[0] counts them) instead of raising kStatusTopkStreamOverflow
                              uint32_t *redo_hdr = nullptr, uint32_t *redo_list = nullptr);
// k > 1 in faiss heap-array order straight from the plan and the tables, no stream and no bound on k or on the admitted
// codes (kernels_heap.hip).  redo_list null: every query of the batch; else the redo_hdr[0] queries listed by
// launch_heap_replay, and the launch's last workgroup re-zeroes redo_hdr[0..1].  heap_ws: heap_scan_ws_bytes of scratch.
bool heap_scan_lds_tier(int code_size, int k);
size_t heap_scan_ws_bytes(int code_size, int k, int nq);
hipError_t launch_heap_scan(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int k,
                            uint32_t *redo_hdr, const uint32_t *redo_list, float *heap_ws, float *dist, int64_t *labels,
                            const ScanFilter &fmask = ScanFilter()); // a filter: the filtered form, as launch_scan
// range search (kernels_range.hip): the scan's plan, table and filter mask as launch_scan takes them, every
// query cut into nsplit slices.  count: slices [nq * nsplit + 1] (zeroed here) = the codes with dist < radius in every
// slice, *total (device, zeroed here) their 64-bit sum, *kernel_name the form that ran.  After launch_scan_excl_u32 over
// slices: lims [nq + 1] = every query's first place, and fill writes hit r of a slice at bases[slice] + r, in scan order.
hipError_t launch_range_count(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int nsplit,
                              int seg_len_hint, float radius, uint32_t *slices, unsigned long long *total,
                              const ScanFilter &fmask, const char **kernel_name);
hipError_t launch_range_lims(hipStream_t s, const uint32_t *bases, int nq, int nsplit, uint64_t *lims);
hipError_t launch_range_fill(hipStream_t s, const IvfTables &t, const float *luts, const PlanView &p, int nsplit,
                             int seg_len_hint, float radius, const uint32_t *bases, float *dist, int64_t *labels,
                             const ScanFilter &fmask);
// keys -> (distance, label) through the plan; also emits signed-orderable keys when out_keys != null
hipError_t launch_select(hipStream_t s, const IvfTables &t, const PlanView &p, const uint64_t *keys, int k, float *dist,
                         int64_t *labels, int64_t *out_keys);
// same, reading signed-orderable keys (after a cross-shard MIN)
hipError_t launch_resolve(hipStream_t s, const IvfTables &t, const PlanView &p, const int64_t *skeys, int k, float *dist,
                          int64_t *labels);
// HNSW walk, one wavefront per query (hnswalg.cpp:48-109,227-234)
hipError_t launch_coarse(hipStream_t s, const GraphTables &g, const float *xq, int nq, int nprobe, int ef,
                         uint32_t *coarse_ids, float *coarse_dists, uint32_t *visited_scratch,
                         size_t visited_words_per_slot, int nslots, uint32_t *status, uint32_t *next_query,
                         size_t visited_bytes = 0, bool *visited_zero = nullptr, // in/out: the whole scratch is zero
                         // queries the fast form cannot finish (> 64 exact ties at the efSearch boundary) are listed in
                         // redo_list [nq] and walked again by launch_coarse_redo, which launch_coarse ends with;
                         // next_query must be followed by three more words (the list's header: length, the redo
                         // launch's counter, its exit count); tail_bitmaps [tail_slots][words] zero on entry and on
                         // exit (walk_set.h TailSpill).  counters_clean (in/out): the four words are zero -- the redo
                         // launch's last wavefront leaves them so, and the launcher then skips its memset
                         uint32_t *redo_list = nullptr, uint32_t *tail_bitmaps = nullptr, int tail_slots = 0,
                         bool *counters_clean = nullptr);
hipError_t launch_coarse_redo(hipStream_t s, const GraphTables &g, const float *xq, int nq, int nprobe, int ef,
                              uint32_t *coarse_ids, float *coarse_dists, uint32_t *visited_scratch,
                              size_t visited_words_per_slot, uint32_t *status, uint32_t *redo_hdr, uint32_t *redo_list,
                              uint32_t *tail_bitmaps, int tail_slots);
// (coarse_slots_for, the wavefront slots the walk keeps resident for a given ef: walk_form.h)
// one workgroup per query on the fat graph (small batches: the reference's one-query-per-call drivers)
bool coarse_latency_supported(const GraphTables &g, int ef);
size_t coarse_latency_fat_bytes(const GraphTables &g);
hipError_t launch_build_fat(hipStream_t s, const GraphTables &g, float *fat);
hipError_t launch_coarse_latency(hipStream_t s, const GraphTables &g, const float *xq, int nq, int nprobe, int ef,
                                 uint32_t *coarse_ids, float *coarse_dists, uint32_t *status,
                                 uint64_t *zero_keys = nullptr, uint32_t *zero_done = nullptr, // [nq] words to clear
                                 uint32_t *redo_hdr = nullptr, uint32_t *redo_list = nullptr); // zeroed header: see launch_coarse
// bits of the device status word
constexpr uint32_t kStatusHnswTieOverflow = 1u; // latency walk on the synchronous host-pointer path only: the call repeats itself (capi_search.cpp)
constexpr uint32_t kStatusTopkStreamOverflow = 2u;
// synthetic corpus: uniform bytes from a counter hash; ids = running index
// construction side (kernels_encode.hip): IndexIVF_HNSW.cpp:75-121
hipError_t launch_madd_rows(hipStream_t s, const float *a, float bf, const float *table, const uint32_t *idx, float *c,
                            size_t n, int d);
hipError_t launch_pq_encode(hipStream_t s, const float *r, const float *cb, uint8_t *codes, size_t n, int d, int M);
hipError_t launch_pq_decode(hipStream_t s, const uint8_t *codes, const float *cb, float *dec, size_t n, int d, int M);
hipError_t launch_norm_codes(hipStream_t s, const float *rec, const float *ntab, uint8_t *norm_codes, float *norms_out,
                             size_t n, int d);
// code-book training (kernels_train.hip): the update half of a Lloyd iteration (the assignment half is
// launch_pq_encode), and OPQ's X^T Y on the matrix cores (chunks of kXtyChunk points, partials [nchunks][d][d])
constexpr int kXtyChunk = 2048;
hipError_t launch_lloyd_update(hipStream_t s, const float *x, const uint8_t *assign, float *cb, size_t n, int d, int M);
hipError_t launch_xty(hipStream_t s, const float *X, const float *Y, float *partials, float *C, size_t n, int d);
// Lloyd k-means of the coarse centroids (kernels_kmeans.hip): counts + objective partials per tile of kKmeansTile points,
// an exclusive scan, a stable sort of the point ids by cluster (LSD radix, 8 bits per pass; *sorted = ids_a or ids_b),
// the means in member order and the in-order split of empty clusters.  hist: [256][ceil(n / kKmeansTile)].
constexpr int kKmeansTile = 4096;
hipError_t launch_kmeans_count(hipStream_t s, const uint32_t *assign, const float *dist, size_t n, uint32_t nc,
                               uint32_t *cnt, double *part, uint32_t *status);
hipError_t launch_scan_u32(hipStream_t s, const uint32_t *in, uint32_t *out, size_t len);
hipError_t launch_sort_by_key(hipStream_t s, const uint32_t *keys, size_t n, int key_bits, uint32_t *ids_a, uint32_t *ids_b,
                              uint32_t *hist, uint32_t **sorted);
// the same sort applied to the permutation `start` (ids_a, ids_b or null = the identity): sorting by a minor key and
// then, from its result, by a major key gives the stable order by (major, minor)
hipError_t launch_sort_by_key_from(hipStream_t s, const uint32_t *keys, size_t n, int key_bits, const uint32_t *start,
                                   uint32_t *ids_a, uint32_t *ids_b, uint32_t *hist, uint32_t **sorted);
hipError_t launch_kmeans_means(hipStream_t s, const float *x, size_t n, const uint32_t *members, const uint32_t *start,
                               const uint32_t *cnt, float *c, size_t nc, int d);
hipError_t launch_kmeans_split(hipStream_t s, float *c, const uint32_t *pairs, size_t npairs, int d);
// exact k-nearest-neighbour tables on the matrix cores (kernels_knn.hip); part = [nsplit][nq][k] u64 workspace
inline int knn_splits_for(size_t nq, size_t nx) { return sweep_splits_for(nq, nx, 128); } // nx >= 1
hipError_t launch_knn_norms(hipStream_t s, const float *x, float *out, size_t n, int d);
hipError_t launch_knn(hipStream_t s, const float *Q, const float *X, const float *qn, const float *xn, size_t nq, size_t nx,
                      int d, int k, int mode, int nsplit, unsigned long long *part, uint32_t *ids, float *dists); // mode: IVFHNSW_KNN_*
// the insertion loop behind the neighbour table (kernels_graph.hip).  forward: node c's links out of row c
// of the IVFHNSW_KNN_EARLIER table into fwd [n][M] (slots beyond fcnt[c] hold n) and deg[t] += 1 for every link to t
// (deg [n + 1] zeroed before).  fold: pairs = the slots 0 .. n * M - 1 of fwd sorted stably by their content, roff
// [n + 1] = the exclusive scan of deg; writes counts [n], links [n][maxM] and the longest reverse list into *longest
// (zeroed before).
size_t graph_forward_lds_bytes(int d, int ncand);
size_t graph_fold_lds_bytes(int d, int maxM);
hipError_t launch_graph_forward(hipStream_t s, const float *x, const uint32_t *table, size_t n, int d, int M, int ncand,
                                uint32_t *fwd, uint8_t *fcnt, uint32_t *deg);
hipError_t launch_graph_fold(hipStream_t s, const float *x, const uint32_t *fwd, const uint8_t *fcnt, const uint32_t *roff,
                             const uint32_t *pairs, size_t n, int d, int M, int maxM, uint8_t *counts, uint32_t *links,
                             uint32_t *longest);
// Grouping construction (IndexIVF_HNSW_Grouping.cpp:43-157)
hipError_t launch_group_table(hipStream_t s, int mode, const float *vectors, const uint32_t *centroid_idx,
                              const uint32_t *nn, const float *alphas, const float *cv_in, float *out, size_t ngroups,
                              int nsubc, int d);
size_t group_points_lds_bytes(int nsubc, int d);
hipError_t launch_group_points(hipStream_t s, int mode, const float *vectors, const uint32_t *centroid_idx,
                               const float *table, const float *cv_norms, const unsigned long long *offsets,
                               const float *x, float *out_num, float *out_den, uint32_t *out_sub, size_t ngroups,
                               int nsubc, int d);
hipError_t launch_group_alpha(hipStream_t s, const unsigned long long *offsets, const float *num, const float *den,
                              float *alphas, size_t ngroups);
hipError_t launch_group_rows(hipStream_t s, const unsigned long long *offsets, const uint32_t *sub, uint32_t *rows,
                             size_t ngroups, int nsubc);
// nbrows[i][j] = qrows[links[i][j]] for j < counts[i], zero otherwise (GraphTables::nbrows)
// row_err: [n] every row's error code (walk_err_code)
hipError_t launch_build_nbrows(hipStream_t s, const GraphTables &g, uint8_t *nbrows, uint32_t *nbnorms, int nb_rows,
                               uint32_t *links_c, const uint16_t *row_err);
hipError_t launch_fill_bytes(hipStream_t s, uint8_t *dst, size_t nbytes, uint64_t seed);
hipError_t launch_fill_iota(hipStream_t s, uint32_t *dst, size_t n, uint32_t first);
hipError_t launch_fill_lists(hipStream_t s, const IvfTables &t, uint8_t *codes, uint8_t *norm_codes, uint32_t *ids,
                             uint64_t seed_codes, uint64_t seed_norms);
// exact re-rank against the uint8 base store (kernels_rerank.hip): rows [count] at src_stride -> the store's layout at dst;
// then for nq queries the k best of kc candidate labels by (exact distance, label), empty slots FLT_MAX / -1
hipError_t launch_rerank_permute(hipStream_t s, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t count, int d);
size_t rerank_lds_bytes(int kc, int d);
hipError_t launch_rerank(hipStream_t s, const uint8_t *base, uint64_t n, int d, const float *queries,
                         const int64_t *cand, size_t nq, int kc, int k, float *dist, int64_t *labels);
// exact brute-force search of the store on the int8 matrix cores (kernels_exact.hip).  Qp: [nq][d] queries
// in the store's byte order (launch_rerank_permute), d % 16 == 0, d <= 256, 1 <= k <= 100; part: [nsplit][nq][k] u64
// workspace; writes the k nearest rows of every query ascending by (distance, label), padded with FLT_MAX / -1
inline int exact_rows_per_block(int k) { return k <= 32 ? 128 : 64; }
inline int exact_splits_for(size_t nq, size_t nx, int k) { return sweep_splits_for(nq, nx, exact_rows_per_block(k)); }
// cols: the column map of a base filter (sweep_plan_math.h SweepCols).  Masked: data = the pass words of
// the nx rows; Indirect: data = the passing row numbers ascending and nx = their number (nx == 0: only padding is written)
hipError_t launch_exact_search(hipStream_t s, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t nx, int d, int k,
                               int nsplit, unsigned long long *part, float *dists, int64_t *labels, const SweepCols &cols = {});
// exact range search (kernels_exact.hip): the same sweep with the fixed gate dist < thr (int32, thr >= 0),
// one launch for the nq queries Qp [nq][d] (permuted) that are queries [q_off, q_off + nq) of the call, q_off % 32 == 0.
// count (fill = false): slices[(q_off + q) * nsplit + split] = the rows of the split that pass, *total (device) += their
// 64-bit sum; neither is zeroed here.  fill: slices holds the exclusive scan of the counts (launch_scan_excl_u32); hit r of
// a slice goes to dist / labels [bases[slice] + r], ascending label; nothing is written at or beyond out_cap.
// map (nullable; then every tile is visited): [ceil(total queries / 32)][nsplit][exact_range_map_words] words, one bit
// per 2^map_shift tiles of 32 columns; the count form writes every word the fill form of the same arguments reads.
constexpr int kExactRangeMaxShift = 20;
inline int exact_range_map_words(size_t nx, int nsplit, int map_shift) { return sweep_map_words(nx, nsplit, map_shift); }
hipError_t launch_exact_range(hipStream_t s, bool fill, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t q_off, size_t nx,
                              int d, int thr, int nsplit, uint32_t *slices, unsigned long long *total, uint32_t *map,
                              int map_shift, float *dist, int64_t *labels, size_t out_cap, const SweepCols &cols = {});
// the base filter of the exact calls (kernels_exact_filter.hip).  words: [sweep_pass_words(n)] = the label
// bitmap bits [bit_words] (null = the empty set) cut or zero-extended to n rows, inverted with deny, bits at or beyond n
// zero; *count (zeroed here) = the rows that pass.  rows: the passing row numbers ascending, [*count]; cnt: workspace of
// sweep_pass_words(n) + 1 words, part: append_scan_parts of that.
hipError_t launch_pass_words(hipStream_t s, const uint32_t *bits, size_t bit_words, uint64_t n, int deny, uint32_t *words,
                             unsigned long long *count);
hipError_t launch_pass_rows(hipStream_t s, const uint32_t *words, uint64_t n, uint32_t *cnt, uint32_t *part, uint32_t *rows);
// Base filter slots: the exact sweeps with a row set per query, resolved per 32-row strip.
// launch_strip_plan: the strip plan of a chunk of m queries from their slot bytes d_slots [m] and the holder's table
// [kStripNone + 1] into plan (sweep_strip_plan_bytes(bound) bytes, bound >= sweep_strip_bound(m)); *sp = its views.
// launch_rerank_permute_rows: launch_rerank_permute whose row r comes from row row_src[r] of src (negative: row 0).
// launch_exact_search_strips / launch_exact_range_strips: the sweeps over the gathered queries Qp [bound * 32][d], one
// launch per form in `forms` (bit kSweepCols*), results at the queries' own places; part: [nsplit][bound * 32][k].
hipError_t launch_strip_plan(hipStream_t s, const uint8_t *d_slots, size_t m, const StripCols *table, void *plan, size_t bound,
                             StripPlan *sp);
hipError_t launch_rerank_permute_rows(hipStream_t s, const uint8_t *src, size_t src_stride, uint8_t *dst, size_t count, int d,
                                      const int32_t *row_src);
hipError_t launch_exact_search_strips(hipStream_t s, const uint8_t *Qp, const uint8_t *X, size_t nq, size_t bound, int d, int k,
                                      int nsplit, unsigned long long *part, float *dists, int64_t *labels, const StripPlan &sp,
                                      unsigned forms, const StripWin *win = nullptr);
hipError_t launch_exact_range_strips(hipStream_t s, bool fill, const uint8_t *Qp, const uint8_t *X, size_t bound, size_t q_off,
                                     size_t nx, int d, int thr, int nsplit, uint32_t *slices, unsigned long long *total,
                                     uint32_t *map, int map_shift, float *dist, int64_t *labels, size_t out_cap,
                                     const StripPlan &sp, unsigned forms, const StripWin *win = nullptr);
// Base tags (kernels_exact_filter.hip): a uint16 per row of the store, and the exact sweeps with a tag per query.
// launch_base_tags_apply: tags[rows[i]] = vals[i] for rows[i] < n; *conflict (zeroed here) != 0 when a row was given two
// different tags.  launch_base_tags_index: the rows sorted stably by tag (*sorted = ids_a or ids_b [n]; keys [n], hist as
// launch_sort_by_key's), off [kTagValues + 1] their starts per tag, stats[0] = the tags with rows, stats[1] = the most
// rows of one tag.  launch_tag_strip_plan: the strip plan of a chunk of m <= kExactChunk queries from their tags d_tags [m]
// into plan (sweep_tag_plan_bytes(bound) bytes, bound >= sweep_tag_strip_bound(m, tags in use)): every strip carries its
// own entry, the Dense strips of the untagged queries first, then the Indirect ones; work: tag_plan_work_words(m) words.
hipError_t launch_base_tags_apply(hipStream_t s, const uint32_t *rows, const uint16_t *vals, size_t cnt, uint64_t n, uint16_t *tags,
                                  uint32_t *conflict);
hipError_t launch_base_tags_index(hipStream_t s, const uint16_t *tags, uint64_t n, uint32_t *keys, uint32_t *ids_a, uint32_t *ids_b,
                                  uint32_t *hist, uint32_t *off, uint32_t *stats, uint32_t **sorted);
size_t tag_plan_work_words(size_t m);
hipError_t launch_tag_strip_plan(hipStream_t s, const uint16_t *d_tags, size_t m, const TagRows &tr, void *plan, size_t bound,
                                 uint32_t *work, StripPlan *sp);
// Base values (kernels_exact_filter.hip): a uint32 per row of the store, and the exact sweeps with an
// interval per query.  launch_base_values_apply: vals[rows[i]] = v[i] for rows[i] < n; *conflict (zeroed here) != 0 when a
// row was given two different values.  launch_base_values_index: all rows sorted stably by value (*sorted = ids_a or ids_b
// [n]; hist as launch_sort_by_key's).  launch_value_windows: win[q] = the window of query q's interval qr[2q], qr[2q + 1]
// in vr's row order (sweep_value_window; no value array: every row holds 0xffffffff).  launch_value_strip_plan: the strip
// plan of a chunk of m <= kExactChunk queries from their intervals d_ranges [2 m] into plan (sweep_value_plan_bytes(bound)
// bytes, bound >= sweep_value_strip_bound(m)): the Dense strips of the queries whose window is the whole store first, then
// the others in the order of their windows' starts, 32 to a strip whose entry spans their windows, *win the windows of its
// rows (the last arguments of the strip sweeps); work: value_plan_work_words(m) words.
// launch_range_by_label: the tot results dist / labels of an exact range search whose lims [nq + 1] are in device memory,
// gathered into out_d / out_l in (query, label) order; work: range_by_label_work_words(tot) words.
hipError_t launch_base_values_apply(hipStream_t s, const uint32_t *rows, const uint32_t *v, size_t cnt, uint64_t n, uint32_t *vals,
                                    uint32_t *conflict);
hipError_t launch_base_values_index(hipStream_t s, const uint32_t *vals, uint64_t n, uint32_t *ids_a, uint32_t *ids_b, uint32_t *hist,
                                    uint32_t **sorted);
hipError_t launch_value_windows(hipStream_t s, const uint32_t *d_ranges, size_t m, const ValueRows &vr, StripWin *win);
size_t value_plan_work_words(size_t m);
hipError_t launch_value_strip_plan(hipStream_t s, const uint32_t *d_ranges, size_t m, const ValueRows &vr, void *plan, size_t bound,
                                   uint32_t *work, StripPlan *sp, const StripWin **win);
size_t range_by_label_work_words(size_t tot);
hipError_t launch_range_by_label(hipStream_t s, const uint64_t *d_lims, size_t nq, size_t tot, const float *dist, const int64_t *labels,
                                 float *out_d, int64_t *out_l, uint32_t *work);
// appends to the inverted lists (kernels_append.hip) and to the sub-groups of Grouping lists (3.12); the
// arithmetic and the workspace sizes are update_math.h's.  count: cnt[list_idx[i]] += 1 and, with sub_idx, sizes2[list][sub]
// += 1 (cnt null: check only); a list id >= nc or a sub-group id >= nsubc raises *status.  tables: own[c] = old length +
// cnt[c] of the owned lists, then cnt and own ([nc + 1] each, slot nc zero) become their exclusive scans nstart / lstart in
// place; part: append_scan_parts(nc + 1) words.  layout: nl.goff / nl.loff and tile_first (append_tile_words words).
// merge, after layout: the old rows into the new arrays nl.  scatter, after merge: the batch's rows (perm = the ids sorted
// stably by list, or by (list, sub-group)) behind the old rows of their lists or sub-groups.  sg null: IVFADC lists.
constexpr int kAppendTileRows = 2048;
struct SubGroups { // a Grouping append: the batch's sub-group ids, the old sizes table, and launch_grouping_prefix's sums
    uint32_t nsubc;
    const uint32_t *sub_idx, *sizes, *pre_old, *pre_new;
};
hipError_t launch_append_count(hipStream_t s, const uint32_t *list_idx, const uint32_t *sub_idx, size_t n, uint32_t nc,
                               uint32_t nsubc, uint32_t *cnt, uint32_t *sizes2, uint32_t *status);
hipError_t launch_append_tables(hipStream_t s, const IvfTables &t, uint32_t *cnt, uint32_t *own, uint32_t *part);
hipError_t launch_append_layout(hipStream_t s, const IvfTables &t, const uint32_t *nstart, const uint32_t *lstart,
                                uint32_t *tile_first, const NewLists &nl);
hipError_t launch_append_merge(hipStream_t s, const IvfTables &t, const uint32_t *nstart, const uint32_t *lstart,
                               const uint32_t *tile_first, const SubGroups *sg, const NewLists &nl);
hipError_t launch_append_scatter(hipStream_t s, const IvfTables &t, const uint32_t *perm, const uint32_t *list_idx, size_t n,
                                 const uint32_t *nstart, const uint32_t *lstart, const SubGroups *sg, const uint8_t *codes,
                                 const uint8_t *norm_codes, const uint32_t *ids, const NewLists &nl);
// prefix, after tables: pre_old / pre_new [nc * nsubc] = exclusive prefix sums of sizes / sizes2 inside every list the
// batch touches (kernels_add_groups.hip)
hipError_t launch_grouping_prefix(hipStream_t s, const uint32_t *nstart, const uint32_t *sizes, const uint32_t *sizes2,
                                  uint32_t *pre_old, uint32_t *pre_new, uint32_t nc, uint32_t nsubc);
// nl.goff / nl.loff from the exclusive scan delta of the rows each list gains (grow) or loses; lstart: the new local starts
// of an append, null = they move by delta too (a removal)
hipError_t launch_update_offsets(hipStream_t s, const IvfTables &t, const uint32_t *delta, const uint32_t *lstart, bool grow,
                                 const NewLists &nl);
// exclusive scan of a [len] in place with the scan above; part: append_scan_parts(len) words
hipError_t launch_scan_excl_u32(hipStream_t s, uint32_t *a, size_t len, uint32_t *part);
// removal by label from an unsharded handle (kernels_remove.hip).  max: atomicMax of the labels into
// *out.  mark: from bits, the label set (launch_remove_bits below), mask [ceil(n_local / kRemoveTileRows) *
// kRemoveTileRows / 64] (bit r = row r is removed) and keep [one per tile] = rows each tile keeps.  counts: rem [nc + 1]
// (slot nc zero) = codes removed per list, also into rem_out when non-null; sizes != null (Grouping): sizes2 [nc * nsubc]
// = the sub-group sizes after the removal.  compact, after rem and keep are scanned (rscan, kscan): nl.goff / nl.loff and the
// surviving rows, in order, into the new arrays nl.
constexpr int kRemoveTileRows = 2048;
hipError_t launch_remove_max(hipStream_t s, const uint32_t *labels, size_t n, uint32_t *out);
hipError_t launch_remove_mark(hipStream_t s, const IvfTables &t, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                              unsigned long long *mask, uint32_t *keep);
hipError_t launch_remove_counts(hipStream_t s, const IvfTables &t, const unsigned long long *mask, const uint32_t *sizes,
                                uint32_t *sizes2, int nsubc, uint32_t *rem, uint32_t *rem_out);
hipError_t launch_remove_compact(hipStream_t s, const IvfTables &t, uint64_t n_local, const unsigned long long *mask,
                                 const uint32_t *rscan, const uint32_t *kscan, const NewLists &nl);
// the label bitmap of every call that takes a label set (capi_labels.cpp): bits [max_label / 32 + 1 words] zeroed, then
// the bit of every label set
hipError_t launch_remove_bits(hipStream_t s, const uint32_t *labels, size_t n, uint32_t max_label, uint32_t *bits);
// upsert (kernels_upsert.hip): a removal and an append of an unsharded IVFADC handle in one rebuild, from
// removal's mask / kscan / rscan and append's nstart / perm.  bits: launch_remove_bits that raises *status when a label
// comes twice.  layout: nl.goff / nl.loff and tile_first [ceil(n_local / kRemoveTileRows) + 1] = the old list of every
// source tile's first row.  compact, after layout: the surviving rows, one contiguous range per (source tile, list)
// segment.  scatter: the batch's rows behind the surviving rows of their lists; it writes no byte compact writes.
hipError_t launch_upsert_bits(hipStream_t s, const uint32_t *labels, size_t n, uint32_t max_label, uint32_t *bits, uint32_t *status);
hipError_t launch_upsert_layout(hipStream_t s, const IvfTables &t, uint64_t n_local, const uint32_t *rscan, const uint32_t *nstart,
                                uint32_t *tile_first, const NewLists &nl);
hipError_t launch_upsert_compact(hipStream_t s, const IvfTables &t, uint64_t n_local, const unsigned long long *mask,
                                 const uint32_t *kscan, const uint32_t *nstart, const uint32_t *tile_first, const NewLists &nl);
hipError_t launch_upsert_scatter(hipStream_t s, const IvfTables &t, const uint32_t *perm, const uint32_t *list_idx, size_t n,
                                 const uint32_t *nstart, const uint32_t *rscan, const uint8_t *codes, const uint8_t *norm_codes,
                                 const uint32_t *ids, const NewLists &nl);
// search filter (kernels_filter.hip): mask [ceil(n_local / 64)] words, bit r = row r passes: its id is in the
// label bitmap (bits null = the empty set), or with deny is not; rows at or beyond n_local are 0.  *count (zeroed here) = the
// rows that pass.
hipError_t launch_filter_mark(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                              int deny, unsigned long long *mask, unsigned long long *count);
// the same for every filter slot of a handle in ONE pass over the ids: plane s < nplanes of planes, stride64
// 64-bit words apart, is the mask of slot s -- all zero where the slot is not set (set[s] 0) -- and counts[s] (the first
// kFilterSlots words zeroed here) the rows that pass it.
constexpr int kFilterSlots = 32;
struct FilterSlotSets {
    const uint32_t *bits[kFilterSlots]; // the slot's label bitmap, null = the empty set
    uint32_t max_label[kFilterSlots];
    uint8_t set[kFilterSlots], deny[kFilterSlots];
};
hipError_t launch_filter_mark_slots(hipStream_t s, const uint32_t *ids, uint64_t n_local, const FilterSlotSets &sets,
                                    uint32_t nplanes, unsigned long long *planes, uint64_t stride64,
                                    unsigned long long *counts);
// Row tags (kernels_filter.hip).  scatter: table[labels[i]] = tags[i], i < n, into a table that spans every
// label given; *conflict (zeroed here) is non-zero afterwards iff a label was given two different tags.  gather:
// row_tags[r] = ids[r] < table_n ? table[ids[r]] : 0xffff for r < n_local (n_local = 0: the one element it always has).
// count: *count (zeroed here) = rows whose tag equals `tag` (equal), or differs from it.
hipError_t launch_tags_scatter(hipStream_t s, const uint32_t *labels, const uint16_t *tags, size_t n, uint16_t *table,
                               uint32_t *conflict);
hipError_t launch_tags_gather(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint16_t *table, uint64_t table_n,
                              uint16_t *row_tags);
hipError_t launch_tags_count(hipStream_t s, const uint16_t *row_tags, uint64_t n_local, uint32_t tag, bool equal,
                             unsigned long long *count);
// Row values (kernels_filter.hip), as the three above with a uint32 per label and per row: none is
// 0xffffffff, and count: *count (zeroed here) = rows whose value lies in [lo, hi], unsigned and inclusive (lo > hi: none).
hipError_t launch_values_scatter(hipStream_t s, const uint32_t *labels, const uint32_t *values, size_t n, uint32_t *table,
                                 uint32_t *conflict);
hipError_t launch_values_gather(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint32_t *table, uint64_t table_n,
                                uint32_t *row_values);
hipError_t launch_values_count(hipStream_t s, const uint32_t *row_values, uint64_t n_local, uint32_t lo, uint32_t hi,
                               unsigned long long *count);
// Tag AND value: *count (zeroed here) = rows whose tag passes `tag` (0xffff: every row) and whose value
// lies in [lo, hi].  A null row array: every row untagged / without a value.
hipError_t launch_tag_values_count(hipStream_t s, const uint16_t *row_tags, const uint32_t *row_values, uint64_t n_local,
                                   uint32_t tag, uint32_t lo, uint32_t hi, unsigned long long *count);
// additions to a Grouping index (kernels_add_groups.hip): its codes go in with the append launchers above.
// add_groups: *status (0xffffffff before) = the lowest g whose list holds codes; list_idx[p] = cidx[group of point p];
// the table rows of G groups (nn always; alpha and the inter-centroid row -- inter_src, or computed when it is null --
// for groups with points); out[i] = table[rows[i]] for rows of nsubc words
hipError_t launch_groups_empty(hipStream_t s, const uint64_t *goff, const uint32_t *cidx, size_t ngroups, uint32_t nc,
                               uint32_t *status);
hipError_t launch_groups_point_lists(hipStream_t s, const unsigned long long *off, const uint32_t *cidx, size_t G,
                                     uint32_t *list_idx);
hipError_t launch_groups_rows(hipStream_t s, const uint32_t *cidx, const unsigned long long *off, const uint32_t *nn_src,
                              const float *alpha_src, const float *inter_src, const float *vectors, int d, uint32_t nsubc,
                              size_t G, uint32_t *nn_dst, float *alpha_dst, float *inter_dst);
hipError_t launch_gather_rows(hipStream_t s, const uint32_t *table, const uint32_t *rows, size_t nrows, uint32_t nsubc,
                              uint32_t *out);
// reconstruction of stored rows (kernels_recon.hip), unsharded handles.  rows: out [n][d] = the ROTATED-
// space vector of resident row rows[i] (anchor + decoded code, one add per component; V = the quantizer's vectors, g null
// = IVFADC); a row outside [0, n_local) is an empty slot: d floats of kReconEmptyBits.  refill: the empty slots of out
// once more (behind launch_opq, which has no rule for them).  resolve_rows: signed result keys of the plan p ->
// the resident row each came from, -1 for an unfilled slot.
constexpr uint32_t kReconEmptyBits = 0x7fc00000u;
hipError_t launch_recon_rows(hipStream_t s, const IvfTables &t, const GroupTables *g, const float *V, uint64_t n_local,
                             const int64_t *rows, size_t n, float *out);
hipError_t launch_recon_refill(hipStream_t s, uint64_t n_local, const int64_t *rows, size_t n, int d, float *out);
hipError_t launch_resolve_rows(hipStream_t s, const PlanView &p, const int64_t *skeys, int k, int64_t *rows);
// locate (same file): hit, one pass over ids [n_local]: an id whose bit is set in bits ([0, max_label]) is looked up in
// sorted [n] (the request's labels ascending, repeats allowed) and its FIRST place p gets lo[p] = min(lo[p], row),
// cnt[p] += 1 (lo 0xffffffff, cnt 0 before).  gather: sorted[j] = labels[perm[j]].  scatter: request perm[j] receives the
// answer of the first place of its label: rows (-1 = none) and counts (nullable); *missing (nullable, zeroed before) +=
// the requests without a row.
hipError_t launch_locate_gather(hipStream_t s, const uint32_t *labels, const uint32_t *perm, size_t n, uint32_t *sorted);
hipError_t launch_locate_hit(hipStream_t s, const uint32_t *ids, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                             const uint32_t *sorted, size_t n, uint32_t *lo, uint32_t *cnt);
hipError_t launch_locate_scatter(hipStream_t s, const uint32_t *sorted, const uint32_t *perm, size_t n, const uint32_t *lo,
                                 const uint32_t *cnt, int64_t *rows, uint32_t *counts, unsigned long long *missing);
// sum of PlanHdr.total / nseg over the batch into out[0], out[1]
hipError_t launch_plan_totals(hipStream_t s, const PlanHdr *hdr, int nq, unsigned long long *out);

} // namespace ivfhnsw_gpu_impl
