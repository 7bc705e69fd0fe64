// What the sources of the C ABI (capi_*.cpp) share: error reporting, the growing device / pinned buffers, the handle
// itself with the one list of its device buffers, and the host helpers more than one subject needs.  Private to the
// library: not installed, nothing outside csrc/ includes it.  The ABI functions take their C linkage from their
// declarations in ivfhnsw_hip.h.
#pragma once
#include "../../include/ivfhnsw_hip.h"
#include "ivfhnsw_kernels.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <cmath>
#include <cstddef>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <unordered_map>
#include <vector>

namespace ivfhnsw_gpu_impl {

// records the message ivfhnsw_gpu_last_error returns on this thread; returns code (capi_handle.cpp)
int fail(int code, const char *fmt, ...) __attribute__((format(printf, 2, 3)));

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t e_ = (expr);                                                                              \
        if (e_ != hipSuccess)                                                                                \
            return fail(e_ == hipErrorOutOfMemory ? IVFHNSW_ERR_NOMEM : IVFHNSW_ERR_HIP, "%s: %s (%s:%d)",   \
                        #expr, hipGetErrorString(e_), __FILE__, __LINE__);                                   \
    } while (0)

// A device allocation that only ever grows.
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes)
            return IVFHNSW_OK;
        release();
        HIP_TRY(hipMalloc(&p, need ? need : 1));
        bytes = need;
        return IVFHNSW_OK;
    }
    void release()
    {
        if (p)
            (void)hipFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

// A DevBuf of one scope: whatever it holds when the scope ends is freed.  A function that builds new state beside what
// the handle has installed keeps it in these, and when nothing can fail any more gives each to its handle member; the
// member's earlier allocation is then this scope's to free.  Every early return frees what was built so far.
struct ScopedBuf : DevBuf {
    ScopedBuf() = default;
    ScopedBuf(const ScopedBuf &) = delete;
    ScopedBuf &operator=(const ScopedBuf &) = delete;
    ~ScopedBuf() { release(); }
    void install(DevBuf &member) { std::swap(static_cast<DevBuf &>(*this), member); }
};

// A label set a handle keeps (the filter, each filter slot): its bitmap over [0, max_label], so that an update can judge
// the rows of its new arrays, and what the set's own calls report.  mode -1 = no set.  Not copied: a view takes the
// fields it reads (follow_parent), never the buffer.
struct LabelSet {
    DevBuf bits;
    uint32_t max_label = 0;
    bool has_bits = false; // false = the empty set (bits unallocated)
    int mode = -1;
    uint64_t pass = 0; // rows of the resident lists that pass
    LabelSet() = default;
    LabelSet(const LabelSet &) = delete;
    LabelSet &operator=(const LabelSet &) = delete;
    const uint32_t *bitmap() const { return has_bits ? bits.as<uint32_t>() : nullptr; }
    // the set of n labels whose bitmap was built in fresh (capi_labels.cpp labels_bitmap); fresh leaves with the earlier one
    void install(ScopedBuf &fresh, size_t n, uint32_t max_label_, int mode_, uint64_t pass_)
    {
        fresh.install(bits);
        max_label = n ? max_label_ : 0;
        has_bits = n != 0;
        mode = mode_;
        pass = pass_;
    }
    void drop() // no label set
    {
        bits.release();
        max_label = 0;
        has_bits = false;
        mode = -1;
        pass = 0;
    }
};

// A base filter slot (capi_base_filter.cpp): a set of row numbers of the store as set_base_filter keeps
// its one -- pass words, and where few rows pass (has_rows) their ascending list.  mode -1 = not set.
struct BaseSlot {
    DevBuf words, rows;
    int mode = -1;
    uint64_t pass = 0;
    bool has_rows = false;
    BaseSlot() = default;
    BaseSlot(const BaseSlot &) = delete;
    BaseSlot &operator=(const BaseSlot &) = delete;
};

// Pinned, device-visible host memory that only ever grows (the small-batch entry point reads queries and writes
// results through it: no staging copies on the latency path).
struct HostBuf {
    void *p = nullptr;
    size_t bytes = 0;
    int ensure(size_t need)
    {
        if (need <= bytes)
            return IVFHNSW_OK;
        release();
        HIP_TRY(hipHostMalloc(&p, need ? need : 1, hipHostMallocDefault));
        bytes = need;
        return IVFHNSW_OK;
    }
    void release()
    {
        if (p)
            (void)hipHostFree(p);
        p = nullptr;
        bytes = 0;
    }
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};

struct StageEvent {
    int stage;
    hipEvent_t a, b;
};

// The handle's w_status buffer.  check_status reads `bits`; the rest are counters that live on the device between
// launches and that the launch which used them leaves zero.  The launchers take the address of a member and reach its
// neighbours from there, hence the asserts.
struct StatusWords {
    uint32_t bits;            // kStatus* (ivfhnsw_kernels.h)
    uint32_t walk_next;       // the walk's query counter (launch_coarse: next_query, followed by the redo header)
    uint32_t redo_len;        // the walk's redo header: queries on the redo list,
    uint32_t redo_next;       // ... the redo launch's counter,
    uint32_t redo_exits;      // ... its exit count
    uint32_t heap_redo_len;   // heap-order queries whose candidate stream overflowed (heap_scan_kernel redoes them),
    uint32_t heap_redo_exits; // ... that launch's exit count
    uint32_t pad;
};
static_assert(offsetof(StatusWords, redo_len) == offsetof(StatusWords, walk_next) + 4 &&
                  offsetof(StatusWords, redo_next) == offsetof(StatusWords, walk_next) + 8 &&
                  offsetof(StatusWords, redo_exits) == offsetof(StatusWords, walk_next) + 12,
              "launch_coarse: next_query is followed by the three words of the redo header");
static_assert(offsetof(StatusWords, heap_redo_exits) == offsetof(StatusWords, heap_redo_len) + 4, "launch_heap_scan: redo_hdr[0..1]");
static_assert(offsetof(StatusWords, bits) == 0 && sizeof(StatusWords) == 8 * sizeof(uint32_t), "8 words, bits first");

// What the host knows about the walk's scratch between calls (walk_scratch, capi_search.cpp; the launchers update the
// two flags through the pointers they take).
struct WalkScratch {
    bool zero = false;          // every byte of w_visited is zero (the walk's overflow bitmaps, kernels_hnsw.hip)
    void *zero_ptr = nullptr;   // ... of this allocation
    size_t zero_bytes = 0;
    bool counters_clean = true; // StatusWords walk_next .. redo_exits are zero (ivfhnsw_gpu_create clears them, the redo launch's last wavefront restores it)
};

} // namespace ivfhnsw_gpu_impl

using namespace ivfhnsw_gpu_impl;

// Every device buffer of the handle, named ONCE: this list is the handle's DevBuf members, what ivfhnsw_gpu_destroy
// frees and what ivfhnsw_gpu_memory_bytes sums (ivfhnsw_gpu::for_each_devbuf).  A new feature adds its buffers here and
// nowhere else.  The pinned HostBufs p_in / p_out are not in it: they are not HBM.
#define IVFHNSW_GPU_DEVBUFS(X) \
    X(goff) X(loff) X(cnorm) X(pqc) X(ntab) X(opq_at) X(opq_a) X(codes) X(ncodes) X(ids) /* index tables */ \
    X(g_alpha) X(g_nn) X(g_sizes) X(g_inter) /* Grouping tables */ \
    X(q_counts) X(q_links) X(q_vectors) X(q_qrows) X(q_nbrows) X(q_nbnorms) X(q_fat) X(q_links_c) X(q_rowerr) /* quantizer */ \
    X(e_pqc) X(e_ntab) X(e_a) X(e_at) X(e_x) X(e_idx) X(e_dist) X(e_res) X(e_tmp) X(e_codes) X(e_ncodes) /* code books, encode */ \
    X(t_x) X(t_y) X(t_cb) X(t_assign) X(t_part) X(t_c) /* pq_train, xty */ \
    X(k_q) X(k_x) X(k_qn) X(k_xn) X(k_part) X(k_ids) X(k_dists) /* knn */ \
    X(km_x) X(km_c) X(km_assign) X(km_dist) X(km_cnt) X(km_start) X(km_ids) X(km_ids2) X(km_hist) X(km_part) X(km_status) X(km_pairs) /* kmeans */ \
    X(gb_table) X(gb_fwd) X(gb_fcnt) X(gb_deg) X(gb_roff) X(gb_ids) X(gb_ids2) X(gb_hist) X(gb_stat) X(gb_counts) X(gb_links) /* build_graph */ \
    X(cg_q) X(cg_cidx) X(cg_ids) X(cg_dists) X(gc_nn) X(cg_cvn) X(cg_tab) X(cg_tab2) X(cg_off) X(cg_alpha2) X(cg_sub) /* add_group */ \
    X(base_rows) X(base_stage) /* uint8 base of the re-rank, rows permuted (kernels_rerank.hip); a view reads its parent's */ \
    X(r_q) X(r_cand) X(r_dist) X(r_lab) /* staging of the host-pointer re-rank */ \
    X(ex_q) X(ex_part) X(ex_raw) X(ex_dist) X(ex_lab) /* exact_search: permuted queries, per-split partial tables; staging of the host form */ \
    X(ap_idx) X(ap_ids) X(ap_codes) X(ap_ncodes) X(ap_cnt) X(ap_own) X(ap_part) X(ap_status) X(ap_perm) X(ap_perm2) X(ap_hist) X(ap_tiles) /* append_ivf, add */ \
    X(gp_sub) X(gp_sizes) X(gp_pre_old) X(gp_pre_new) X(gp_rows) X(gp_gather) X(ga_cidx) X(ga_off) X(ga_nn) X(ga_alpha) X(ga_inter) X(ga_status) /* append_grouping, add_groups */ \
    X(rm_labels) X(rm_bits) X(rm_mask) X(rm_keep) X(rm_rem) X(rm_out) X(rm_part) X(rm_status) X(rm_sizes) /* remove_ids */ \
    X(f_mask) X(f_count) /* set_filter: the pass mask, the count's word (the kept label bitmap: filter.bits) */ \
    X(fs_planes) X(fs_count) X(fs_qslots) /* filter slots: the planes (their label bitmaps: slots[].bits), staging of counts and a host call's slot bytes (a _tags call's shorts, a _values call's pairs, a _tags_values call's both) */ \
    X(tg_table) X(tg_rows) /* row tags: a uint16 per label value, a uint16 per resident row */ \
    X(vl_table) X(vl_rows) /* row values: a uint32 per label value, a uint32 per resident row */ \
    X(bf_words) X(bf_rows) X(bf_own) X(bf_count) /* set_base_filter: pass words, pass rows; a list this handle was forced to build; the count's word */ \
    X(bs_table) X(bs_plan) X(bs_qslots) /* base filter slots: the table the strips read (their words and rows: bslots[]); a call's strip plans (a _tags call's too), a host call's slot bytes (a _tags call's shorts) */ \
    X(bt_tags) X(bt_rows) X(bt_off) X(bt_work) /* base tags: a uint16 per store row, the tagged rows by (tag, row), their starts per tag; a call's plan workspace */ \
    X(bv_vals) X(bv_rows) X(bv_work) /* base values: a uint32 per store row, all rows by (value, row); a call's plan workspace */ \
    X(w_xq) X(w_luts) X(w_segs) X(w_lpos) X(w_hdr) X(w_keys) X(w_cid) X(w_cd) X(w_qsd) X(w_totals) X(w_visited) X(w_status) X(w_stream) X(w_slen) X(w_tail) X(w_redo) X(w_hredo) X(w_heap) /* per-batch workspace */ \
    X(rg_dist) X(rg_lab) X(rg_slices) X(rg_part) X(rg_lims) /* range_search: the results it holds; slice counts, scan partials, lims staging */ \
    X(xr_dist) X(xr_lab) X(xr_slices) X(xr_part) X(xr_map) X(xr_lims) X(xr_tot) /* exact_range_search: the results it holds; slice counts, scan partials, tile map, lims staging, total */ \
    X(lc_bits) X(lc_labels) X(lc_sorted) X(lc_perm) X(lc_perm2) X(lc_hist) X(lc_lo) X(lc_cnt) X(lc_rows) X(lc_counts) X(lc_scalar) /* locate: label bitmap, the sorted request, answers, staging */ \
    X(rc_rows) X(rc_y) X(rc_out) X(sr_keys) X(sr_rows) /* reconstruct: staged rows, the ROTATED chunk of an OPQ call, host-form output; search_reconstruct's keys and rows */ \
    X(s_q) X(s_cid) X(s_cd) X(s_dist) X(s_lab) X(s_keys) X(s_len) /* staging of the host-pointer entry points */

struct ivfhnsw_gpu {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    bool is_view = false; // ivfhnsw_gpu_create_view: tables belong to the parent, workspace and stream are its own

#define IVFHNSW_X(name) DevBuf name;
    IVFHNSW_GPU_DEVBUFS(IVFHNSW_X)
#undef IVFHNSW_X
    template <class F> void for_each_devbuf(F &&f)
    {
#define IVFHNSW_X(name) f(name);
        IVFHNSW_GPU_DEVBUFS(IVFHNSW_X)
#undef IVFHNSW_X
        f(filter.bits);
        for (LabelSet &s : slots)
            f(s.bits);
        for (BaseSlot &s : bslots) {
            f(s.words);
            f(s.rows);
        }
    }
    HostBuf p_in, p_out; // pinned: small batches of the host-pointer entry point

    IvfTables t{};
    const float *opq_A = nullptr; // the OPQ matrix as uploaded, row major (t.opq_At is its transpose): reconstruct's way back
    bool has_ivf = false;
    uint64_t n_local = 0;
    GroupTables g{};
    bool has_group = false;
    GraphTables gr{};
    bool has_graph = false;
    size_t e_d = 0, e_M = 0;
    bool e_opq = false, has_codebooks = false;
    uint64_t base_n = 0;
    size_t base_d = 0;
    ivfhnsw_gpu *parent = nullptr;

    // the label filter (capi_filter.cpp).  filter.mode -1 = none.  fmask is what the scans read: the
    // handle's own f_mask, on a view the mask its parent held when follow_parent ran (with the parent's mode and pass).
    LabelSet filter;
    const uint32_t *fmask = nullptr;

    // filter slots (capi_filter.cpp): up to IVFHNSW_FILTER_SLOTS label sets, named per query by the _slots
    // calls.  fs is what their scans read (its `slots` stays null: the bytes travel with the call): fs.nplanes planes of
    // fs.stride words in the handle's own fs_planes, on a view the planes its parent held when follow_parent ran.  A slot
    // that is not set has, where it has a plane, a zero one.
    SlotMask fs{nullptr, 0, 0, nullptr};
    LabelSet slots[IVFHNSW_FILTER_SLOTS];

    // row tags (capi_filter.cpp): tg_table holds a uint16 per label value below tg_labels (0 = no table),
    // tg_rows the tag of every resident row, re-derived by every set_tags and every in-place update.  row_tags is what the
    // _tags scans read: the handle's own tg_rows, on a view what its parent held when follow_parent ran; null = no table,
    // every row untagged.
    uint64_t tg_labels = 0;
    const uint16_t *row_tags = nullptr;

    // row values (capi_filter.cpp), the same with a uint32: vl_table holds one per label value below
    // vl_labels (0 = no table), vl_rows the value of every resident row; row_values is what the _values scans read, null =
    // no table, every row without a value.
    uint64_t vl_labels = 0;
    const uint32_t *row_values = nullptr;

    // the base filter of the exact calls (capi_base_filter.cpp), on the handle that holds the store: a view
    // reads its parent's at the call.  bf_mode -1 = none.  bf_words: one pass bit per row; bf_rows (bf_has_rows): the
    // bf_pass passing row numbers ascending.  bf_gen counts the changes, so that the list a handle built for itself because
    // "exact_filter_form" 1 asked for one the holder does not keep (bf_own, of holder bf_own_of at bf_own_gen) is not
    // used for a later filter.
    int bf_mode = -1;
    uint64_t bf_pass = 0;
    bool bf_has_rows = false;
    uint64_t bf_gen = 0, bf_own_gen = 0;
    const ivfhnsw_gpu *bf_own_of = nullptr;

    // base filter slots (capi_base_filter.cpp), on the handle that holds the store, beside and independent
    // of its one base filter: a view reads its parent's at the call.  bs_table: the kStripNone + 1 entries the strips of an
    // exact _slots call read (form, words or rows, columns), rewritten whenever a slot or the option "exact_filter_form"
    // changes; gone with the store, written again by the first call that needs it.
    BaseSlot bslots[IVFHNSW_FILTER_SLOTS];

    // base tags (capi_base_tags.cpp), on the handle that holds the store, independent of the base filter, of
    // its slots and of the index's row tags: a view reads its parent's at the call.  bt_tags (null = no tag array, every row
    // untagged): a uint16 per store row; bt_rows: the bt_tagged tagged row numbers ordered by (tag, row); bt_off
    // [kTagValues + 1]: tag t's rows are bt_rows [bt_off[t], bt_off[t + 1]).  All three rebuilt by every set_base_tags.
    uint64_t bt_tagged = 0;
    uint32_t bt_in_use = 0, bt_max_rows = 0; // tags that have rows; the most rows of one tag

    // base values (capi_base_values.cpp), on the handle that holds the store, independent of the base filter,
    // of its slots, of the base tags and of the index's row values: a view reads its parent's at the call.  bv_vals (null = no
    // value array, every row valueless): a uint32 per store row; bv_rows: ALL row numbers ordered by (value, row), the
    // bv_valued rows that hold a value first.  Both rebuilt by every set_base_values.
    uint64_t bv_valued = 0;

    // one large batch as two uneven parts on two streams (ivfhnsw_gpu_search_dev): the second part runs on this view
    ivfhnsw_gpu *split_view = nullptr;
    hipEvent_t split_fork = nullptr, split_join = nullptr;
    // ... and both parts' ADC tables are built beside the walks on a stream of the lowest priority (search_dev_split)
    hipStream_t early_stream = nullptr;
    hipEvent_t early_ready[2] = {nullptr, nullptr}; // per part: its rotated queries are there (OPQ only)
    hipEvent_t early_done[2] = {nullptr, nullptr};  // per part: its tables are written
    bool early_failed = false;                      // the stream could not be created: today's launches, not tried again
    bool last_split = false;
    uint32_t *status_shared = nullptr; // the internal split view raises its status bits in the PARENT's word (no merge launch)
    size_t last_parts[2] = {0, 0}; // queries in the two parts of the last search_dev call (second 0 = one part)
    int split_pm = 0; // permille of a large batch in its first part; 0 = one part (ivfhnsw_gpu_set_batch_split)
    WalkScratch walk;
    int opt_scan_pipe = -1;    // ivfhnsw_gpu_set_option "scan_pipe"
    int opt_exact_splits = -1; // ... "exact_splits"
    int opt_exact_range_map = -1; // ... "exact_range_map"
    int opt_exact_filter_form = -1; // ... "exact_filter_form"

    // the plan the last search_dev chunk left (remember_plan, capi_search.cpp)
    int last_nq = 0, last_max_seg = 0;
    const char *last_scan_kernel = "";
    bool last_stream = false; // ... and a candidate stream (k > 1, heap_order)
    bool last_range = false;  // ... left by a range search: it serves last_scan_counts, not resolve_keys

    // the results of the last range search (capi_range.cpp): rg_total entries of rg_dist / rg_lab
    bool rg_valid = false;
    uint64_t rg_total = 0;
    // ... and of the last exact range search (capi_exact.cpp): xr_total entries of xr_dist / xr_lab
    bool xr_valid = false;
    uint64_t xr_total = 0;

    int profiling = 0; // 0 off, 1 every stage, 2 only the scan (an event pair costs ~7 us of stream time)
    std::vector<StageEvent> pending;
    std::vector<hipEvent_t> pool;
    double stage_ms[IVFHNSW_STAGE_COUNT] = {0};
    uint64_t stage_n[IVFHNSW_STAGE_COUNT] = {0};
};

namespace ivfhnsw_gpu_impl {

// ---- capi_handle.cpp
int bind(ivfhnsw_gpu *h);
int upload(DevBuf &b, const void *src, size_t bytes);
hipEvent_t take_event(ivfhnsw_gpu *h);
int drain_events(ivfhnsw_gpu *h);
// After a stream sync: did any kernel flag something it could not represent?
int check_status(ivfhnsw_gpu *h);

// the word the kernels of this handle raise status bits in
inline StatusWords *status_words(ivfhnsw_gpu *h) { return h->w_status.as<StatusWords>(); }
inline uint32_t *status_word(ivfhnsw_gpu *h) { return h->status_shared ? h->status_shared : &status_words(h)->bits; }

// the scan plan in the handle's workspace, as the launchers take it
inline PlanView plan_of(const ivfhnsw_gpu *h, int max_seg, size_t nq)
{
    return {h->w_segs.as<Seg>(), h->w_lpos.as<uint32_t>(), h->w_hdr.as<PlanHdr>(), max_seg, (int)nq};
}

// a view reads its parent's tables: what create_view copies once and a split batch before every call (uploads and
// in-place updates since the view's creation included)
void follow_parent(ivfhnsw_gpu *view, const ivfhnsw_gpu *parent);

// The opening of every call that changes the tables a handle holds: not through a view, the device bound and, with
// need_ivf, lists present ("<who> before upload_ivf").  Each caller adds its own further conditions behind it.
enum TableChange { kUploads, kAppends, kRemovals }; // kUploads: the message carries no "<who>: "
int table_change_guard(ivfhnsw_gpu *h, TableChange what, const char *who, bool need_ivf);

// h->t's pointers to the five list arrays and n_local follow the handle's buffers
void point_at_lists(ivfhnsw_gpu *h, uint64_t n_local);

// ---- capi_labels.cpp: what the calls that take a set of uint32 labels share
// One device word as a kernel's answer: the word is set to `init` bytes, `launch(word)` puts its work on the handle's
// stream, and the word comes back in *out.  Returns with the stream drained.
int run_with_word(ivfhnsw_gpu *h, DevBuf &word, int init, const std::function<hipError_t(uint32_t *)> &launch, uint32_t *out);
// "<who>: null labels" for n > 0 labels without a pointer and, of a call that takes a mode, one that is neither allow
// nor deny
int label_args_guard(size_t n, const uint32_t *labels, const char *who, const int *mode = nullptr);
// Host labels [n] on their way to the device: copied into stage (grown here; n = 0: untouched) on the handle's stream,
// and their maximum (0 for none) into *max_label where the caller wants it.
int labels_from_host(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, DevBuf &stage, uint32_t *max_label);
// The maximum of device labels [n] (0 for none), through `word` (grown to one word here).  n > 0: drains the stream.
int labels_max_dev(ivfhnsw_gpu *h, DevBuf &word, size_t n, const uint32_t *d_labels, uint32_t *max_label);
// the words of a bitmap over [0, max_label]
inline size_t label_bitmap_words(uint32_t max_label) { return (size_t)max_label / 32 + 1; }
// The bitmap of device labels [n] over [0, max_label] into bits (grown here), on the handle's stream.  n = 0, the empty
// set, has no bitmap: bits is left alone.
int labels_bitmap(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, DevBuf &bits);
// The opening of the calls that set or clear a filter: on the handle that holds what the filter is marked over, not on
// a view of it, the device bound and, with need_upload, that upload made ("<who> before upload_ivf" / "... upload_base").
enum FilterKind { kIndexFilter, kBaseFilter };
int filter_holder_guard(ivfhnsw_gpu *h, FilterKind kind, const char *who, bool need_upload);
// what filter_info, filter_slot_info and base_filter_info answer (each pointer nullable): a set's mode and its passing
// rows, or -1 and unset_pass where there is none
int label_set_info(int set_mode, uint64_t pass, uint64_t unset_pass, uint64_t total, int *mode, uint64_t *rows_passing,
                   uint64_t *rows_total);

// ---- capi_filter.cpp
// The pass mask of h's filter over ids [n_local] into mask (allocated here) and the rows that pass into *pass.  Returns
// with the stream drained; the handle is not touched.
int filter_mark_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &mask, uint64_t *pass);
void filter_drop(ivfhnsw_gpu *h); // the handle holds no filter afterwards (buffers released)
// Filter slots.  The words between two planes over n_local rows: whole 64-bit words, never zero.
inline uint64_t slot_plane_stride(uint64_t n_local) { return std::max<uint64_t>((n_local + 63) / 64, 1) * 2; }
// Every installed slot of h judged over ids [n_local] in one pass: planes (allocated here, h->fs.nplanes of them at
// slot_plane_stride(n_local)) and the rows that pass each.  Returns with the stream drained; the handle is not touched.
int slots_mark_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &planes, uint64_t *pass);
void slots_drop(ivfhnsw_gpu *h); // the handle holds no slot afterwards (buffers released)
// what a _slots entry point checks first, behind the plain call's own guard
int slots_call_guard(const ivfhnsw_gpu *h, const char *who, bool tags = false); // tags: the same for a _tags entry point
int slots_call_guard(const ivfhnsw_gpu *h, const char *who, int kind); // ... by QueryPick::kind(): 0 _slots, 1 _tags, 2 _values, 3 _tags_values
// the slot bytes of a host call: each is below IVFHNSW_FILTER_SLOTS or IVFHNSW_SLOT_NONE
int slots_bytes_guard(size_t nq, const uint8_t *query_slots, const char *who);
// (every uint16 is a tag: the host form of a _tags call has nothing to check there)
// Row tags.  The tag of ids [n_local] from h's table into row_tags (allocated here, max(n_local, 1)
// elements).  Returns with the stream drained; the handle is not touched.
int tags_gather_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &row_tags);
void tags_drop(ivfhnsw_gpu *h); // the handle holds no tags afterwards (buffers released)
// Row values: the same two for the uint32 of every row.
int values_gather_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &row_values);
void values_drop(ivfhnsw_gpu *h);

// The five arrays that make up the resident lists, built BESIDE the handle's: an in-place update fills a fresh set and
// installs it when it is complete and the stream has drained, so that on any error the handle's tables are the ones it
// had.  The destructor frees what was not installed -- after install, the handle's previous arrays.
struct ListArrays {
    DevBuf goff, loff, codes, ncodes, ids;
    DevBuf fmask; // the handle's filter judged over the new ids (mark_filter); installed with them
    uint64_t fpass = 0;
    DevBuf fplanes; // ... and its filter slots, every plane in one pass
    uint64_t fs_pass[IVFHNSW_FILTER_SLOTS] = {};
    DevBuf ftags; // ... and its row tags, gathered from the tag table
    DevBuf fvalues; // ... and its row values, gathered from the value table
    ListArrays() = default;
    ListArrays(const ListArrays &) = delete;
    ListArrays &operator=(const ListArrays &) = delete;
    ~ListArrays() { release(); }
    int allocate(size_t nc, uint64_t n_local, size_t M)
    {
        int rc;
        if ((rc = goff.ensure((nc + 1) * sizeof(uint64_t))) || (rc = loff.ensure(nc * sizeof(uint32_t))) ||
            (rc = codes.ensure(n_local * M)) || (rc = ncodes.ensure(n_local)) || (rc = ids.ensure(n_local * sizeof(uint32_t))))
            return rc;
        return IVFHNSW_OK;
    }
    NewLists view(uint64_t n_local) const // what the update launchers fill
    {
        return {goff.as<uint64_t>(), loff.as<uint32_t>(), codes.as<uint8_t>(), ncodes.as<uint8_t>(), ids.as<uint32_t>(), n_local};
    }
    // The one place an update re-marks the filter: rows move and new rows must be judged.  Called when the new ids are
    // complete and BEFORE install, so that a failure here leaves tables, filter, slots, tags and values as they were.
    // No filter, no slot, no tag table and no value table: nothing.
    int mark_filter(ivfhnsw_gpu *h, uint64_t n_local)
    {
        int rc;
        if (h->tg_labels && (rc = tags_gather_rows(h, ids.as<uint32_t>(), n_local, ftags)))
            return rc;
        if (h->vl_labels && (rc = values_gather_rows(h, ids.as<uint32_t>(), n_local, fvalues)))
            return rc;
        if (h->fs.nplanes && (rc = slots_mark_rows(h, ids.as<uint32_t>(), n_local, fplanes, fs_pass)))
            return rc;
        if (h->filter.mode < 0)
            return IVFHNSW_OK;
        return filter_mark_rows(h, ids.as<uint32_t>(), n_local, fmask, &fpass);
    }
    void release()
    {
        for (DevBuf *b : {&goff, &loff, &codes, &ncodes, &ids, &fmask, &fplanes, &ftags, &fvalues})
            b->release();
    }
    void install(ivfhnsw_gpu *h, uint64_t n_local)
    {
        if (h->filter.mode >= 0) {
            std::swap(h->f_mask, fmask);
            h->fmask = h->f_mask.as<uint32_t>();
            h->filter.pass = fpass;
        }
        if (h->fs.nplanes) {
            std::swap(h->fs_planes, fplanes);
            h->fs.planes = h->fs_planes.as<uint32_t>();
            h->fs.stride = (uint32_t)slot_plane_stride(n_local);
            for (int s = 0; s < IVFHNSW_FILTER_SLOTS; s++)
                h->slots[s].pass = fs_pass[s];
        }
        if (h->tg_labels) {
            std::swap(h->tg_rows, ftags);
            h->row_tags = h->tg_rows.as<uint16_t>();
        }
        if (h->vl_labels) {
            std::swap(h->vl_rows, fvalues);
            h->row_values = h->vl_rows.as<uint32_t>();
        }
        std::swap(h->goff, goff);
        std::swap(h->loff, loff);
        std::swap(h->codes, codes);
        std::swap(h->ncodes, ncodes);
        std::swap(h->ids, ids);
        release(); // the old arrays
        point_at_lists(h, n_local);
    }
};

struct StageScope {
    ivfhnsw_gpu *h;
    hipStream_t s; // the handle's stream, or the one the stage's launches really go to (a split call's early tables)
    StageEvent ev{};
    bool on;
    StageScope(ivfhnsw_gpu *h_, int stage, hipStream_t s_ = nullptr)
        : h(h_), s(s_ ? s_ : h_->stream), on(h_->profiling == 1 || (h_->profiling == 2 && stage == IVFHNSW_STAGE_SCAN))
    {
        if (!on)
            return;
        ev.stage = stage;
        ev.a = take_event(h);
        ev.b = take_event(h);
        (void)hipEventRecord(ev.a, s);
    }
    ~StageScope()
    {
        if (!on)
            return;
        (void)hipEventRecord(ev.b, s);
        h->pending.push_back(ev);
    }
};

// candidate-stream entries per query kept for the heap-order replay (k > 1)
constexpr uint32_t kHeapStreamCap = 8192;

constexpr int kSplitAuto = 1000; // the first part's share follows the call's walk : table + plan + scan estimate

// Batches beyond kMaxBatch queries are processed in slices so that the per-batch workspace (16 KB of table per
// query at PQ16, plus the plan) stays bounded; the multi-GPU resolve step needs the whole plan, so it is limited
// to one slice.
constexpr size_t kMaxBatchAll = 1 << 17;

// ---- capi_search.cpp: the stages of one search_dev chunk that range search (capi_range.cpp) runs as well
// What one search call asks of the stages below it; the default is a plain search_dev / coarse_dev call.
// One part of a split call builds its ADC tables early: on `stream`, beside the walks, instead of behind its own walk.
struct EarlyTables {
    hipStream_t stream; // the handle's helper stream; it already waits for the call's fork
    hipEvent_t ready;   // recorded behind the part's rotation (OPQ), which the tables are built from
    hipEvent_t done;    // recorded behind the table launch; the part's scan waits for it
};

struct SearchCall {
    uint32_t *status_out = nullptr; // in: pinned word the tail kernel copies the status into (host-pointer path)
    bool defer_redo = false;        // in: the latency walk only flags a tie overflow, the caller repeats the call ...
    bool no_latency = false;        // in: ... with this set, on the throughput walk
    bool wrote_status = false;      // out: the tail kernel wrote *status_out
    const EarlyTables *early = nullptr; // in: the part of a split call that is running (search_dev_split), else null
};

// The tail kernel's per-query meeting words, which the latency walk clears on its way when it runs.
struct WalkClear {
    uint64_t *keys = nullptr; // in
    uint32_t *done = nullptr; // in
    bool cleared = false;     // out
};

// What a _slots, a _tags, a _values or a _tags_values entry point carries beside the plain call's arguments (DESIGN.md
// 3.19, 3.21, 3.24, 3.26): a filter slot byte, a tag or an interval (two uint32: lo, hi) per query, in host or device
// memory as the call's other arrays are.  One of the three at most, except that a tag AND an interval go together.
struct QueryPick {
    const uint8_t *slots = nullptr;
    const uint16_t *tags = nullptr;
    const uint32_t *ranges = nullptr;
    explicit operator bool() const { return slots || tags || ranges; }
    bool both() const { return tags && ranges; }
    int kind() const { return both() ? 3 : ranges ? 2 : tags ? 1 : 0; } // what slots_call_guard is told
    // The arrays of nq queries as they ride in ONE block (the pinned input block, the staging buffer): the pairs first, so
    // that they are 8-byte aligned wherever the block is, the tags of a _tags_values call behind them.
    size_t tags_at(size_t nq) const { return both() ? nq * 2 * sizeof(uint32_t) : 0; }
    size_t bytes(size_t nq) const
    {
        return slots ? nq : (tags ? nq * sizeof(uint16_t) : 0) + (ranges ? nq * 2 * sizeof(uint32_t) : 0);
    }
    // f(source, offset in the block, bytes) for every array the pick holds; stops at the first non-zero result
    template <class F> int each_array(size_t nq, F &&f) const
    {
        int rc = 0;
        if (slots)
            rc = f(static_cast<const void *>(slots), (size_t)0, nq);
        if (!rc && ranges)
            rc = f(static_cast<const void *>(ranges), (size_t)0, nq * 2 * sizeof(uint32_t));
        if (!rc && tags)
            rc = f(static_cast<const void *>(tags), tags_at(nq), nq * sizeof(uint16_t));
        return rc;
    }
    // the same kind of pick with its nq queries' arrays in the block at p / for the queries from q0 on
    QueryPick at(const void *p, size_t nq) const
    {
        return {slots ? static_cast<const uint8_t *>(p) : nullptr,
                tags ? reinterpret_cast<const uint16_t *>(static_cast<const char *>(p) + tags_at(nq)) : nullptr,
                ranges ? static_cast<const uint32_t *>(p) : nullptr};
    }
    QueryPick from(size_t q0) const
    {
        return {slots ? slots + q0 : nullptr, tags ? tags + q0 : nullptr, ranges ? ranges + 2 * q0 : nullptr};
    }
    // the entry point's name: "<call>_slots", "<call>_tags", "<call>_values" or "<call>_tags_values"
    const char *who(const char *slotted, const char *tagged, const char *valued, const char *tag_valued) const
    {
        return both() ? tag_valued : ranges ? valued : tags ? tagged : slotted;
    }
};
// a host call's pick into the handle's staging buffer (fs_qslots), laid out as above; at(h->fs_qslots.p, nq) reads it
int pick_stage_in(ivfhnsw_gpu *h, const QueryPick &pick, size_t nq);

// The arguments of ivfhnsw_gpu_search_dev, handed down as one.
struct SearchArgs {
    size_t nq, k;
    const float *d_queries;
    const uint32_t *d_coarse_ids;
    const float *d_coarse_dists;
    const ivfhnsw_search_params *p;
    float *d_distances;
    int64_t *d_labels, *d_out_keys;
    QueryPick pick{}; // a _slots / _tags / _values / _tags_values call: the slot, tag, interval or both of every query (device memory), else empty
    SearchArgs slice(size_t q0, size_t n, size_t d) const // the same call for queries [q0, q0 + n)
    {
        return {n, k, d_queries + q0 * d, d_coarse_ids ? d_coarse_ids + q0 * p->nprobe : nullptr,
                d_coarse_dists ? d_coarse_dists + q0 * p->nprobe : nullptr, p, d_distances + q0 * k, d_labels + q0 * k,
                d_out_keys, pick.from(q0)};
    }
};

// One chunk on its way through the stages below: its arguments, and what a stage leaves for the later ones.
struct Chunk : SearchArgs {
    int nprobe, max_seg, plan_k;    // chunk_workspace
    bool heap_big;                  // k > 1024: the heap-order scan only (no top-k keys, no stream)
    ScanFilter fmask;               // a label filter, the call's filter slots (3.19), tags (3.21), values (3.24) or both (3.26)
    const float *xq;                // chunk_coarse: the rotated queries, the coarse results,
    const uint32_t *cid;
    const float *cd;
    bool use_tail;                  // ... everything behind them in one launch (chunk_tail),
    WalkClear meet;                 // ... whose meeting words the walk may have cleared
    int nsplit;                     // chunk_plan_table: workgroups per query,
    bool heap, pipe;                // ... heap order with a stream, table and scan in one pipelined kernel
    const EarlyTables *early;       // search_dev_chunk: a split call's part (SearchCall::early); null everywhere else
};

int search_args_guard(const ivfhnsw_gpu *h, const ivfhnsw_search_params *p, size_t k);
int stage_in(ivfhnsw_gpu *h, DevBuf &b, const void *src, size_t bytes);
int stage_out(ivfhnsw_gpu *h, void *dst, const DevBuf &b, size_t bytes);
// results = false: a caller without d_distances / d_labels of [nq][k] (range search sizes its own output)
int chunk_checks(ivfhnsw_gpu *h, const Chunk &c, bool results = true);
int chunk_workspace(ivfhnsw_gpu *h, Chunk &c);
int chunk_coarse(ivfhnsw_gpu *h, Chunk &c, const SearchCall &call);
int chunk_plan_table(ivfhnsw_gpu *h, Chunk &c);

// ---- capi_base_filter.cpp
void base_filter_drop(ivfhnsw_gpu *h); // the handle holds no base filter afterwards (buffers released)
// The column map of an exact call of h on holder b's store and the columns it sweeps (*nx; 0 = nothing passes, no sweep):
// Dense without a base filter, else the form sweep_filter_form picks.  May build h's own list (bf_own) on h's stream.
int base_filter_cols(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, SweepCols *cols, size_t *nx);

// Base filter slots.
void base_slots_drop(ivfhnsw_gpu *h); // the handle holds no base filter slot afterwards (buffers and table released)
// the holder's table from its slots, on its stream, which is drained; nothing to do on a handle without store or table
int base_slots_table_write(ivfhnsw_gpu *h, bool create);
// What an exact _slots call of h on holder b's store sweeps: the table (written here if the holder has none yet) and the
// forms its entries take (bit kSweepCols*; Dense always: "none" may be named).  ERR_STATE with a base filter installed.
int base_slots_call(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const char *who, const StripCols **table, unsigned *forms);

// ---- capi_base_tags.cpp: base tags
void base_tags_drop(ivfhnsw_gpu *h); // the handle holds no base tags afterwards (buffers released)
// What an exact _tags call of h on holder b's store sweeps: the holder's row lists and the tags in use (the strip bound's
// argument).  ERR_STATE with a base filter installed.
int base_tags_call(const ivfhnsw_gpu *b, const char *who, TagRows *tr, size_t *tags_in_use);

// ---- capi_base_values.cpp: base values
void base_values_drop(ivfhnsw_gpu *h); // the handle holds no base values afterwards (buffers released)
// What an exact _values call of h on holder b's store sweeps: the holder's values and row order.  ERR_STATE with a base
// filter installed.
int base_values_call(const ivfhnsw_gpu *b, const char *who, ValueRows *vr);

// ---- capi_range.cpp
void range_drop(ivfhnsw_gpu *h); // the handle holds no range results afterwards (buffers released)

// ---- capi_upload.cpp
int grouping_dedupe_reserve(ivfhnsw_gpu *h);
int grouping_dedupe_dev(ivfhnsw_gpu *h, const uint32_t *d_sizes, const uint32_t *d_nn, int *dedupe);

// ---- capi_build.cpp
int encode_rows(ivfhnsw_gpu *h, size_t m, float *dx, const float *table, const uint32_t *rows);
int encode_groups_impl(ivfhnsw_gpu *h, size_t ngroups, size_t nsubc, const uint32_t *centroid_idx,
                       const uint64_t *offsets, const float *x, size_t efSearch, uint32_t *out_nn_centroid_idxs,
                       float *out_alphas, uint32_t *out_subcentroid_idxs, uint8_t *out_codes, uint8_t *out_norm_codes,
                       bool dev, bool stage);

} // namespace ivfhnsw_gpu_impl
