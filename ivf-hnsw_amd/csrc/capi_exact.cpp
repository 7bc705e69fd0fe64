#include "capi_internal.h"

#include <climits>

// ---------------------------------------------------------------------------------------------------------------------
// Exact brute-force search of the uint8 base store (kernels_exact.hip): the ground truth the drivers
// read as -path_gt (tests/test_ivfhnsw_sift1b.cpp:173-215), computed from the store upload_base left in HBM.

namespace {

// queries per pass of the kernel (kExactChunk: bounds the permuted queries and, with the splits, the partial tables,
// <= kExactPartBytes = 256 MB): sweep_plan_math.h, with the chunk rule of the _tags calls

// What every exact call checks before it touches anything, in this order: the handle; the store (*b: a view searches its
// parent's); the call's own arguments (arg_check() returns their error, or 0); and, when there are queries, the buffers
// (any_null, with the call's text) and the row stride.  nq == 0 passes: the caller returns what its empty call returns.
template <class ArgCheck>
int exact_guard(ivfhnsw_gpu *h, const char *name, size_t nq, size_t row_stride, bool any_null, const char *null_text,
                ArgCheck arg_check, const ivfhnsw_gpu **b)
{
    int rc = bind(h);
    if (rc)
        return rc;
    *b = h->parent ? h->parent : h;
    if (!(*b)->base_n)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_base", name);
    const size_t d = (*b)->base_d;
    if (d > 256)
        return fail(IVFHNSW_ERR_INVALID,
                    "%s on a store of dimension %zu: beyond d = 256 the squared distance can exceed 2^24 and is no longer the "
                    "exact float fvec_L2sqr returns",
                    name, d);
    if ((rc = arg_check()) || nq == 0)
        return rc;
    if (any_null)
        return fail(IVFHNSW_ERR_INVALID, "%s", null_text);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    return IVFHNSW_OK;
}

// A _slots call: the slot byte of every query (device memory once staged), the holder's table and the
// forms its entries take.  A _tags call (3.22): the tag of every query, the holder's row lists and its tags in use; its
// strips are Dense (untagged queries) and Indirect.  A _values call (3.25): the interval of every query and the holder's
// values and row order; its strips are Dense (the whole store) and windowed Indirect.  All null: the plain call.
struct SlotsArg {
    const uint8_t *d_slots = nullptr;
    const StripCols *table = nullptr;
    unsigned forms = 0;
    const uint16_t *d_tags = nullptr;
    TagRows tr;
    size_t tags_in_use = 0;
    const uint32_t *d_ranges = nullptr;
    ValueRows vr;
    explicit operator bool() const { return d_slots || d_tags || d_ranges; }
    // the strips a chunk of m queries can have, and the bytes of its plan
    size_t bound(size_t m) const
    {
        return d_ranges ? sweep_value_strip_bound(m) : d_tags ? sweep_tag_strip_bound(m, tags_in_use) : sweep_strip_bound(m);
    }
    size_t plan_bytes(size_t bound) const
    {
        return d_ranges ? sweep_value_plan_bytes(bound) : d_tags ? sweep_tag_plan_bytes(bound) : sweep_strip_plan_bytes(bound);
    }
};

// the plan of the chunk of m queries from q0 on (ds / dt / dr: the chunk's slot bytes, tags or intervals in device memory);
// *win: the windows of a _values plan's strip rows, else null
int exact_strip_plan(ivfhnsw_gpu *h, const SlotsArg &sl, const uint8_t *ds, const uint16_t *dt, const uint32_t *dr, size_t m,
                     void *plan, size_t bound, StripPlan *sp, const StripWin **win)
{
    *win = nullptr;
    if (dr)
        HIP_TRY(launch_value_strip_plan(h->stream, dr, m, sl.vr, plan, bound, h->bv_work.as<uint32_t>(), sp, win));
    else if (dt)
        HIP_TRY(launch_tag_strip_plan(h->stream, dt, m, sl.tr, plan, bound, h->bt_work.as<uint32_t>(), sp));
    else
        HIP_TRY(launch_strip_plan(h->stream, ds, m, sl.table, plan, bound, sp));
    return IVFHNSW_OK;
}

// what a _tags entry point checks behind the plain call's guard: no base filter installed; the Indirect sweep only where
// a row is tagged
int exact_tags_guard(ivfhnsw_gpu *h, const char *who, SlotsArg *sl)
{
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    const int rc = base_tags_call(b, who, &sl->tr, &sl->tags_in_use);
    sl->forms = 1u << kSweepColsDense | (b->bt_tagged ? 1u << kSweepColsIndirect : 0u);
    return rc;
}

// ... and a _values entry point: the windowed sweep only where a row holds a value
int exact_values_guard(ivfhnsw_gpu *h, const char *who, SlotsArg *sl)
{
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    const int rc = base_values_call(b, who, &sl->vr);
    sl->forms = 1u << kSweepColsDense | (sl->vr.vals ? 1u << kSweepColsIndirect : 0u);
    return rc;
}

// what a _slots entry point checks behind the plain call's guard, before anything is launched or written: no base filter
// installed, and the bytes of a host form
int exact_slots_guard(ivfhnsw_gpu *h, const char *who, size_t nq, const uint8_t *query_slots, bool on_device, SlotsArg *sl)
{
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    int rc = base_slots_call(h, b, who, &sl->table, &sl->forms);
    if (rc == IVFHNSW_OK && !on_device)
        rc = slots_bytes_guard(nq, query_slots, who);
    return rc;
}

// query_slots / query_tags / query_ranges (one of them at most; all null: the plain call): one slot byte, one tag or one
// interval (lo, hi) per query, where the queries are
int exact_impl(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k, float *distances,
               int64_t *labels, bool on_device, const uint8_t *query_slots = nullptr, const uint16_t *query_tags = nullptr,
               const uint32_t *query_ranges = nullptr)
{
    const ivfhnsw_gpu *b;
    auto k_check = [&] { return k < 1 || k > 100 ? fail(IVFHNSW_ERR_INVALID, "exact_search needs 1 <= k <= 100 (k %zu)", k) : 0; };
    int rc = exact_guard(h, "exact_search", nq, row_stride, !queries || !distances || !labels, "null query/result buffer", k_check, &b);
    if (rc || nq == 0)
        return rc;
    const size_t d = b->base_d;
    // under a base filter the columns of the sweep: every row behind the pass words, or the list of passing rows
    SweepCols cols;
    size_t n;
    SlotsArg sl;
    if (query_slots) { // ... and with a slot per query (3.20) each strip's own, from the holder's table
        if ((rc = exact_slots_guard(h, "exact_search_slots", nq, query_slots, on_device, &sl)))
            return rc;
        n = b->base_n;
    } else if (query_tags) { // ... or a tag per query (3.22): each strip's own entry, a tag's row list
        if ((rc = exact_tags_guard(h, "exact_search_tags", &sl)))
            return rc;
        n = b->base_n;
    } else if (query_ranges) { // ... or an interval per query (3.25): each strip's own entry, each row's own window of it
        if ((rc = exact_values_guard(h, "exact_search_values", &sl)))
            return rc;
        n = b->base_n;
    } else if ((rc = base_filter_cols(h, b, &cols, &n)))
        return rc;
    const bool strips = query_slots || query_tags || query_ranges;
    const size_t per_query = query_ranges ? 2 * sizeof(uint32_t) : query_tags ? sizeof(uint16_t) : 1; // bytes of a query's slot, tag or interval

    const size_t first = std::min(nq, kExactChunk);
    const int nsplit = h->opt_exact_splits > 0 ? h->opt_exact_splits : exact_splits_for(first, n, (int)k);
    size_t chunk = kExactPartBytes / ((size_t)nsplit * k * sizeof(uint64_t));
    chunk = std::max<size_t>(128, std::min(kExactChunk, chunk / 128 * 128));
    if (query_tags) { // with many tags the padded rows, not the queries, size the partial tables
        sl.d_tags = query_tags;
        chunk = sweep_tag_chunk(nsplit, k, sl.tags_in_use);
    }
    if (query_ranges) {
        sl.d_ranges = query_ranges;
        chunk = sweep_value_chunk(nsplit, k);
    }
    chunk = std::min(chunk, nq);
    // the rows a chunk is swept as: its queries, or under a strip plan the 32 rows of every strip it can have
    const size_t bound = strips ? sl.bound(chunk) : 0;
    const size_t rows = strips ? bound * 32 : chunk;
    if ((rc = h->ex_q.ensure(rows * d)) || (rc = h->ex_part.ensure((size_t)nsplit * rows * k * sizeof(uint64_t))))
        return rc;
    if (strips && ((rc = h->bs_plan.ensure(sl.plan_bytes(bound))) ||
                   (!on_device && (rc = h->bs_qslots.ensure(chunk * per_query)))))
        return rc;
    if (query_tags && (rc = h->bt_work.ensure(tag_plan_work_words(chunk) * sizeof(uint32_t))))
        return rc;
    if (query_ranges && (rc = h->bv_work.ensure(value_plan_work_words(chunk) * sizeof(uint32_t))))
        return rc;
    if (!on_device && ((rc = h->ex_raw.ensure(chunk * d)) || (rc = h->ex_dist.ensure(chunk * k * sizeof(float))) ||
                       (rc = h->ex_lab.ensure(chunk * k * sizeof(int64_t)))))
        return rc;
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const size_t m = std::min(chunk, nq - q0);
        const uint8_t *src = queries + q0 * row_stride;
        size_t src_stride = row_stride;
        if (!on_device) {
            HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d, src, row_stride, d, m, hipMemcpyHostToDevice, h->stream));
            src = h->ex_raw.as<uint8_t>();
            src_stride = d;
        }
        float *od = on_device ? distances + q0 * k : h->ex_dist.as<float>();
        int64_t *ol = on_device ? labels + q0 * k : h->ex_lab.as<int64_t>();
        if (strips) {
            const uint8_t *ds = query_slots ? query_slots + q0 : nullptr;
            const uint16_t *dt = query_tags ? query_tags + q0 : nullptr;
            const uint32_t *dr = query_ranges ? query_ranges + 2 * q0 : nullptr;
            if (!on_device) {
                HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, ds ? (const void *)ds : dt ? (const void *)dt : dr, m * per_query,
                                       hipMemcpyHostToDevice, h->stream));
                ds = ds ? h->bs_qslots.as<uint8_t>() : nullptr;
                dt = dt ? h->bs_qslots.as<uint16_t>() : nullptr;
                dr = dr ? h->bs_qslots.as<uint32_t>() : nullptr;
            }
            // the chunk's strips, its queries gathered into them in the pass that permutes them, one sweep per form
            StripPlan sp;
            const StripWin *win;
            if ((rc = exact_strip_plan(h, sl, ds, dt, dr, m, h->bs_plan.p, bound, &sp, &win)))
                return rc;
            HIP_TRY(launch_rerank_permute_rows(h->stream, src, src_stride, h->ex_q.as<uint8_t>(), rows, (int)d, sp.strip_rows));
            HIP_TRY(launch_exact_search_strips(h->stream, h->ex_q.as<uint8_t>(), b->base_rows.as<uint8_t>(), m, bound, (int)d, (int)k,
                                               nsplit, h->ex_part.as<unsigned long long>(), od, ol, sp, sl.forms, win));
        } else {
            // the queries in the store's byte order: an integer sum does not care which order, only that it is the same
            HIP_TRY(launch_rerank_permute(h->stream, src, src_stride, h->ex_q.as<uint8_t>(), m, (int)d));
            HIP_TRY(launch_exact_search(h->stream, h->ex_q.as<uint8_t>(), b->base_rows.as<uint8_t>(), m, n, (int)d, (int)k, nsplit,
                                        h->ex_part.as<unsigned long long>(), od, ol, cols));
        }
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(distances + q0 * k, od, m * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(labels + q0 * k, ol, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            // the next chunk reuses the pageable source and the staging buffers
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return IVFHNSW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// Exact range search: count -> prefix -> (one synchronisation: the host sizes the results) -> fill, both
// passes the sweep of exact_mfma_kernel with a fixed gate (exact_range_kernel).

// (float)dist < radius for an integer 0 <= dist < 2^24, as an int32 threshold: dist < thr
int exact_range_threshold(float radius)
{
    if (!(radius > 0.f))
        return 0;
    if (radius > 16777216.f)
        return INT_MAX;
    return (int)ceilf(radius);
}

// what both forms check before they touch anything
int exact_range_guard(ivfhnsw_gpu *h, size_t nq, const void *queries, size_t row_stride, float radius, const void *lims,
                      const void *total)
{
    const ivfhnsw_gpu *b;
    auto radius_check = [&] { return std::isnan(radius) ? fail(IVFHNSW_ERR_INVALID, "exact_range_search: the radius is NaN") : 0; };
    const int rc = exact_guard(h, "exact_range_search", nq, row_stride, !queries || !lims || !total,
                               "exact_range_search: null queries, lims or total", radius_check, &b);
    if (rc == IVFHNSW_OK && nq > kMaxBatchAll)
        return fail(IVFHNSW_ERR_INVALID, "exact_range_search is limited to %zu queries per call", kMaxBatchAll);
    return rc;
}

// a call without queries: lims is the one entry 0 (on the host or on the device), and no results are held
int exact_range_none(ivfhnsw_gpu *h, uint64_t *lims, uint64_t *d_lims, uint64_t *total)
{
    if (lims)
        lims[0] = 0;
    if (d_lims) {
        HIP_TRY(hipMemsetAsync(d_lims, 0, sizeof(uint64_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (total)
        *total = 0;
    h->xr_valid = true;
    h->xr_total = 0;
    return IVFHNSW_OK;
}

// The tile map's granularity: one bit per 2^shift tiles of (32 queries, 32 rows), the finest whose map stays within a
// sixteenth of the store -- or, on a store too small for that, the one word per (32 queries, split) that is the least.
int exact_range_map_shift(size_t nq, size_t n, size_t d, int nsplit, size_t *bytes)
{
    const size_t strips = (nq + 31) / 32;
    int shift = 0;
    for (;; shift++) {
        const size_t words = (size_t)exact_range_map_words(n, nsplit, shift);
        *bytes = strips * nsplit * words * sizeof(uint32_t);
        if (*bytes <= n * d / 16 || words == 1 || shift == kExactRangeMaxShift)
            return shift;
    }
}

// the sweep of one form over every chunk of the call's queries (h->ex_q: all of them, permuted)
// The strip plans of a _slots call, kept for both passes: one per chunk, each of `bound` strips, chunk i's
// gathered queries at row i * bound * 32 of h->ex_q.
struct RangeStrips {
    size_t bound = 0;
    unsigned forms = 0;
    std::vector<StripPlan> plans;
    std::vector<const StripWin *> wins; // a _values call (3.25): the windows of each plan's strip rows, else null
};

int exact_range_pass(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const SweepCols &cols, size_t nx, bool fill, size_t nq, int thr,
                     int nsplit, int map_shift, float *dist, int64_t *labels, size_t out_cap, const RangeStrips *rs = nullptr)
{
    const size_t d = b->base_d;
    StageScope sc(h, fill ? IVFHNSW_STAGE_SELECT : IVFHNSW_STAGE_SCAN); // accounted as range_search accounts its passes
    uint32_t *map = h->opt_exact_range_map ? h->xr_map.as<uint32_t>() : nullptr;
    for (size_t q0 = 0, i = 0; q0 < nq; q0 += kExactChunk, i++) { // (kExactChunk % 128 == 0: a chunk starts a workgroup's strip)
        if (rs)
            HIP_TRY(launch_exact_range_strips(h->stream, fill, h->ex_q.as<uint8_t>() + i * rs->bound * 32 * d, b->base_rows.as<uint8_t>(),
                                              rs->bound, q0, nx, (int)d, thr, nsplit, h->xr_slices.as<uint32_t>(),
                                              h->xr_tot.as<unsigned long long>(), map, map_shift, dist, labels, out_cap, rs->plans[i],
                                              rs->forms, rs->wins[i]));
        else
            HIP_TRY(launch_exact_range(h->stream, fill, h->ex_q.as<uint8_t>() + q0 * d, b->base_rows.as<uint8_t>(),
                                       std::min(kExactChunk, nq - q0), q0, nx, (int)d, thr, nsplit, h->xr_slices.as<uint32_t>(),
                                       h->xr_tot.as<unsigned long long>(), map, map_shift, dist, labels, out_cap, cols));
    }
    return IVFHNSW_OK;
}

// device pointers, the arguments checked (nq > 0)
int exact_range_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, float radius, uint64_t *d_lims,
                    uint64_t *total, const SlotsArg &sl = {})
{
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    const size_t d = b->base_d;
    const int thr = exact_range_threshold(radius);
    int rc;
    SweepCols cols; // the columns of the sweep under a base filter, as in exact_impl
    size_t n = b->base_n;
    if (!sl && (rc = base_filter_cols(h, b, &cols, &n)))
        return rc;
    if (thr == 0 || n == 0) { // nothing is below it, or no row passes the base filter: no sweep
        HIP_TRY(hipMemsetAsync(d_lims, 0, (nq + 1) * sizeof(uint64_t), h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->xr_valid = true;
        h->xr_total = 0;
        *total = 0;
        return IVFHNSW_OK;
    }
    const int nsplit = h->opt_exact_splits > 0 ? h->opt_exact_splits : exact_splits_for(std::min(nq, kExactChunk), n, 1);
    const size_t len = nq * (size_t)nsplit + 1;
    // under a strip plan the rows swept are those of every strip a chunk can have, chunk after chunk
    RangeStrips strips;
    const size_t nchunks = (nq + kExactChunk - 1) / kExactChunk;
    if (sl) {
        strips.bound = sl.bound(std::min(nq, kExactChunk));
        strips.forms = sl.forms;
        strips.plans.resize(nchunks);
        strips.wins.assign(nchunks, nullptr);
    }
    // a _values call: per chunk the strips of its plan that are windowed, read back with the count
    std::vector<uint32_t> win_range(sl.d_ranges ? 2 * nchunks : 0, 0u);
    const size_t rows = sl ? nchunks * strips.bound * 32 : nq;
    const size_t plan_bytes = sl.plan_bytes(strips.bound);
    size_t map_bytes = 0;
    const int map_shift = exact_range_map_shift(rows, n, d, nsplit, &map_bytes);
    if ((rc = h->ex_q.ensure(rows * d)) || (rc = h->xr_slices.ensure(len * sizeof(uint32_t))) ||
        (rc = h->xr_part.ensure(append_scan_parts(len) * sizeof(uint32_t))) ||
        (rc = h->xr_tot.ensure(sizeof(unsigned long long))) || (h->opt_exact_range_map && (rc = h->xr_map.ensure(map_bytes))) ||
        (sl && (rc = h->bs_plan.ensure(nchunks * plan_bytes))) ||
        (sl.d_tags && (rc = h->bt_work.ensure(tag_plan_work_words(std::min(nq, kExactChunk)) * sizeof(uint32_t)))) ||
        (sl.d_ranges && (rc = h->bv_work.ensure(value_plan_work_words(std::min(nq, kExactChunk)) * sizeof(uint32_t)))))
        return rc;
    if (sl) {
        // per chunk: its strips, and its queries gathered into them in the pass that permutes them
        for (size_t q0 = 0, i = 0; q0 < nq; q0 += kExactChunk, i++) {
            StripPlan &sp = strips.plans[i];
            if ((rc = exact_strip_plan(h, sl, sl.d_slots ? sl.d_slots + q0 : nullptr, sl.d_tags ? sl.d_tags + q0 : nullptr,
                                       sl.d_ranges ? sl.d_ranges + 2 * q0 : nullptr, std::min(kExactChunk, nq - q0),
                                       h->bs_plan.as<unsigned char>() + i * plan_bytes, strips.bound, &sp, &strips.wins[i])))
                return rc;
            if (sl.d_ranges)
                HIP_TRY(hipMemcpyAsync(&win_range[2 * i], sp.hdr->lay.range[kSweepColsIndirect], 2 * sizeof(uint32_t),
                                       hipMemcpyDeviceToHost, h->stream));
            sp.map_strip0 = (uint32_t)(i * strips.bound);
            HIP_TRY(launch_rerank_permute_rows(h->stream, d_queries + q0 * row_stride, row_stride,
                                               h->ex_q.as<uint8_t>() + i * strips.bound * 32 * d, strips.bound * 32, (int)d, sp.strip_rows));
        }
    } else {
        HIP_TRY(launch_rerank_permute(h->stream, d_queries, row_stride, h->ex_q.as<uint8_t>(), nq, (int)d));
    }
    const RangeStrips *rs = sl ? &strips : nullptr;
    HIP_TRY(hipMemsetAsync(h->xr_slices.p, 0, len * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->xr_tot.p, 0, sizeof(unsigned long long), h->stream));
    if ((rc = exact_range_pass(h, b, cols, n, false, nq, thr, nsplit, map_shift, nullptr, nullptr, 0, rs)))
        return rc;
    HIP_TRY(launch_scan_excl_u32(h->stream, h->xr_slices.as<uint32_t>(), len, h->xr_part.as<uint32_t>()));
    // the one synchronisation between the passes: the host sizes the results from the count
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, h->xr_tot.p, sizeof(tot), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (tot >= (1ull << 32))
        return fail(IVFHNSW_ERR_INVALID, "exact_range_search: %llu results in one call, the limit is 2^32 - 1 (use a smaller "
                                         "radius or fewer queries per call)", tot);
    // Under a windowed strip the fill pass writes a query's results in (value, row) order: they are then
    // gathered in (query, label) order into a second pair of arrays that replaces the first.
    bool windowed = false;
    for (size_t i = 0; i < win_range.size(); i += 2)
        windowed |= win_range[i + 1] > win_range[i];
    // results: in the buffers the handle holds when they are large enough, else in new ones swapped in when they are full
    DevBuf nd, nl, rd, rl, rwork; // rd, rl: the reordered pair; rwork: the keys and permutations of its two sorts
    auto release = [&] {
        nd.release();
        nl.release();
        rd.release();
        rl.release();
        rwork.release();
    };
    const bool grow = tot * sizeof(float) > h->xr_dist.bytes || tot * sizeof(int64_t) > h->xr_lab.bytes;
    if (grow && ((rc = nd.ensure(tot * sizeof(float))) || (rc = nl.ensure(tot * sizeof(int64_t))))) {
        release();
        return rc;
    }
    // ... and the reordered pair with its workspace, before the fill pass writes anything: a failed allocation leaves the
    // results the handle holds as they were
    if (tot && windowed && ((rc = rd.ensure(tot * sizeof(float))) || (rc = rl.ensure(tot * sizeof(int64_t))) ||
                            (rc = rwork.ensure(range_by_label_work_words(tot) * sizeof(uint32_t))))) {
        release();
        return rc;
    }
    auto fill = [&]() -> int {
        HIP_TRY(launch_range_lims(h->stream, h->xr_slices.as<uint32_t>(), (int)nq, nsplit, d_lims));
        if (tot)
            if (int e = exact_range_pass(h, b, cols, n, true, nq, thr, nsplit, map_shift, grow ? nd.as<float>() : h->xr_dist.as<float>(),
                                         grow ? nl.as<int64_t>() : h->xr_lab.as<int64_t>(), (size_t)tot, rs))
                return e;
        if (tot && windowed) {
            StageScope sc(h, IVFHNSW_STAGE_PLAN); // accounted apart from the two passes: the order of the results
            HIP_TRY(launch_range_by_label(h->stream, d_lims, nq, tot, grow ? nd.as<float>() : h->xr_dist.as<float>(),
                                          grow ? nl.as<int64_t>() : h->xr_lab.as<int64_t>(), rd.as<float>(), rl.as<int64_t>(),
                                          rwork.as<uint32_t>()));
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        return IVFHNSW_OK;
    };
    if ((rc = fill())) {
        release();
        return rc;
    }
    if (rd.p) {
        std::swap(h->xr_dist, rd);
        std::swap(h->xr_lab, rl);
    } else if (grow) {
        std::swap(h->xr_dist, nd);
        std::swap(h->xr_lab, nl);
    }
    release();
    h->xr_valid = true;
    h->xr_total = tot;
    *total = tot;
    return IVFHNSW_OK;
}

} // namespace

int ivfhnsw_gpu_exact_range_search_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, float radius,
                                       uint64_t *d_lims, uint64_t *total)
{
    int rc = exact_range_guard(h, nq, d_queries, row_stride, radius, d_lims, total);
    if (rc)
        return rc;
    if (nq == 0)
        return exact_range_none(h, nullptr, d_lims, total);
    return exact_range_dev(h, nq, d_queries, row_stride, radius, d_lims, total);
}

int ivfhnsw_gpu_exact_range_search(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, float radius,
                                   uint64_t *lims, uint64_t *total)
{
    int rc = exact_range_guard(h, nq, queries, row_stride, radius, lims, total);
    if (rc)
        return rc;
    if (nq == 0)
        return exact_range_none(h, lims, nullptr, total);
    const size_t d = (h->parent ? h->parent : h)->base_d;
    if ((rc = h->ex_raw.ensure(nq * d)) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d, queries, row_stride, d, nq, hipMemcpyHostToDevice, h->stream));
    if ((rc = exact_range_dev(h, nq, h->ex_raw.as<uint8_t>(), d, radius, h->xr_lims.as<uint64_t>(), total)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_exact_range_results(ivfhnsw_gpu *h, uint64_t first, uint64_t count, float *distances, int64_t *labels)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->xr_valid)
        return fail(IVFHNSW_ERR_STATE, "exact_range_results before an exact range search on this handle");
    if (first > h->xr_total || count > h->xr_total - first)
        return fail(IVFHNSW_ERR_INVALID, "exact_range_results: [%llu, %llu + %llu) is beyond the %llu results held",
                    (unsigned long long)first, (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)h->xr_total);
    if (count == 0)
        return IVFHNSW_OK;
    if (distances)
        HIP_TRY(hipMemcpyAsync(distances, h->xr_dist.as<float>() + first, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (labels)
        HIP_TRY(hipMemcpyAsync(labels, h->xr_lab.as<int64_t>() + first, count * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_exact_range_results_dev(ivfhnsw_gpu *h, const float **d_distances, const int64_t **d_labels, uint64_t *total)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->xr_valid)
        return fail(IVFHNSW_ERR_STATE, "exact_range_results_dev before an exact range search on this handle");
    if (d_distances)
        *d_distances = h->xr_total ? h->xr_dist.as<float>() : nullptr;
    if (d_labels)
        *d_labels = h->xr_total ? h->xr_lab.as<int64_t>() : nullptr;
    if (total)
        *total = h->xr_total;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_exact_search(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                             float *distances, int64_t *labels)
{
    return exact_impl(h, nq, queries, row_stride, k, distances, labels, false);
}

int ivfhnsw_gpu_exact_search_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                 float *d_distances, int64_t *d_labels)
{
    return exact_impl(h, nq, d_queries, row_stride, k, d_distances, d_labels, true);
}

// ---- with a base filter slot per query; query_slots == NULL is the plain call

int ivfhnsw_gpu_exact_search_slots(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                                   const uint8_t *query_slots, float *distances, int64_t *labels)
{
    return exact_impl(h, nq, queries, row_stride, k, distances, labels, false, query_slots);
}

int ivfhnsw_gpu_exact_search_slots_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                       const uint8_t *d_query_slots, float *d_distances, int64_t *d_labels)
{
    return exact_impl(h, nq, d_queries, row_stride, k, d_distances, d_labels, true, d_query_slots);
}

int ivfhnsw_gpu_exact_range_search_slots_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride,
                                             const uint8_t *d_query_slots, float radius, uint64_t *d_lims, uint64_t *total)
{
    if (!d_query_slots)
        return ivfhnsw_gpu_exact_range_search_dev(h, nq, d_queries, row_stride, radius, d_lims, total);
    int rc = exact_range_guard(h, nq, d_queries, row_stride, radius, d_lims, total);
    if (rc)
        return rc;
    SlotsArg sl;
    if ((rc = exact_slots_guard(h, "exact_range_search_slots_dev", nq, d_query_slots, true, &sl)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, nullptr, d_lims, total);
    sl.d_slots = d_query_slots;
    return exact_range_dev(h, nq, d_queries, row_stride, radius, d_lims, total, sl);
}

int ivfhnsw_gpu_exact_range_search_slots(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride,
                                         const uint8_t *query_slots, float radius, uint64_t *lims, uint64_t *total)
{
    if (!query_slots)
        return ivfhnsw_gpu_exact_range_search(h, nq, queries, row_stride, radius, lims, total);
    int rc = exact_range_guard(h, nq, queries, row_stride, radius, lims, total);
    if (rc)
        return rc;
    SlotsArg sl;
    if ((rc = exact_slots_guard(h, "exact_range_search_slots", nq, query_slots, false, &sl)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, lims, nullptr, total);
    const size_t d = (h->parent ? h->parent : h)->base_d;
    if ((rc = h->ex_raw.ensure(nq * d)) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))) || (rc = h->bs_qslots.ensure(nq)))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d, queries, row_stride, d, nq, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, query_slots, nq, hipMemcpyHostToDevice, h->stream));
    sl.d_slots = h->bs_qslots.as<uint8_t>();
    if ((rc = exact_range_dev(h, nq, h->ex_raw.as<uint8_t>(), d, radius, h->xr_lims.as<uint64_t>(), total, sl)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// ---- with a base tag per query; query_tags == NULL is the plain call

int ivfhnsw_gpu_exact_search_tags(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                                  const uint16_t *query_tags, float *distances, int64_t *labels)
{
    return exact_impl(h, nq, queries, row_stride, k, distances, labels, false, nullptr, query_tags);
}

int ivfhnsw_gpu_exact_search_tags_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                      const uint16_t *d_query_tags, float *d_distances, int64_t *d_labels)
{
    if (d_query_tags && ((uintptr_t)d_query_tags & 1))
        return fail(IVFHNSW_ERR_INVALID, "exact_search_tags_dev: query tags must be 2-byte aligned");
    return exact_impl(h, nq, d_queries, row_stride, k, d_distances, d_labels, true, nullptr, d_query_tags);
}

int ivfhnsw_gpu_exact_range_search_tags_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride,
                                            const uint16_t *d_query_tags, float radius, uint64_t *d_lims, uint64_t *total)
{
    if (!d_query_tags)
        return ivfhnsw_gpu_exact_range_search_dev(h, nq, d_queries, row_stride, radius, d_lims, total);
    int rc = exact_range_guard(h, nq, d_queries, row_stride, radius, d_lims, total);
    if (rc)
        return rc;
    if ((uintptr_t)d_query_tags & 1)
        return fail(IVFHNSW_ERR_INVALID, "exact_range_search_tags_dev: query tags must be 2-byte aligned");
    SlotsArg sl;
    if ((rc = exact_tags_guard(h, "exact_range_search_tags_dev", &sl)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, nullptr, d_lims, total);
    sl.d_tags = d_query_tags;
    return exact_range_dev(h, nq, d_queries, row_stride, radius, d_lims, total, sl);
}

int ivfhnsw_gpu_exact_range_search_tags(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride,
                                        const uint16_t *query_tags, float radius, uint64_t *lims, uint64_t *total)
{
    if (!query_tags)
        return ivfhnsw_gpu_exact_range_search(h, nq, queries, row_stride, radius, lims, total);
    int rc = exact_range_guard(h, nq, queries, row_stride, radius, lims, total);
    if (rc)
        return rc;
    SlotsArg sl;
    if ((rc = exact_tags_guard(h, "exact_range_search_tags", &sl)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, lims, nullptr, total);
    const size_t d = (h->parent ? h->parent : h)->base_d;
    if ((rc = h->ex_raw.ensure(nq * d)) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))) ||
        (rc = h->bs_qslots.ensure(nq * sizeof(uint16_t))))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d, queries, row_stride, d, nq, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, query_tags, nq * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    sl.d_tags = h->bs_qslots.as<uint16_t>();
    if ((rc = exact_range_dev(h, nq, h->ex_raw.as<uint8_t>(), d, radius, h->xr_lims.as<uint64_t>(), total, sl)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// ---- with an interval of base values per query; query_ranges == NULL is the plain call

int ivfhnsw_gpu_exact_search_values(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                                    const uint32_t *query_ranges, float *distances, int64_t *labels)
{
    return exact_impl(h, nq, queries, row_stride, k, distances, labels, false, nullptr, nullptr, query_ranges);
}

int ivfhnsw_gpu_exact_search_values_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                        const uint32_t *d_query_ranges, float *d_distances, int64_t *d_labels)
{
    if (d_query_ranges && ((uintptr_t)d_query_ranges & 7))
        return fail(IVFHNSW_ERR_INVALID, "exact_search_values_dev: query ranges must be 8-byte aligned");
    return exact_impl(h, nq, d_queries, row_stride, k, d_distances, d_labels, true, nullptr, nullptr, d_query_ranges);
}

int ivfhnsw_gpu_exact_range_search_values_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride,
                                              const uint32_t *d_query_ranges, float radius, uint64_t *d_lims, uint64_t *total)
{
    if (!d_query_ranges)
        return ivfhnsw_gpu_exact_range_search_dev(h, nq, d_queries, row_stride, radius, d_lims, total);
    int rc = exact_range_guard(h, nq, d_queries, row_stride, radius, d_lims, total);
    if (rc)
        return rc;
    if ((uintptr_t)d_query_ranges & 7)
        return fail(IVFHNSW_ERR_INVALID, "exact_range_search_values_dev: query ranges must be 8-byte aligned");
    SlotsArg sl;
    if ((rc = exact_values_guard(h, "exact_range_search_values_dev", &sl)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, nullptr, d_lims, total);
    sl.d_ranges = d_query_ranges;
    return exact_range_dev(h, nq, d_queries, row_stride, radius, d_lims, total, sl);
}

int ivfhnsw_gpu_exact_range_search_values(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride,
                                          const uint32_t *query_ranges, float radius, uint64_t *lims, uint64_t *total)
{
    if (!query_ranges)
        return ivfhnsw_gpu_exact_range_search(h, nq, queries, row_stride, radius, lims, total);
    int rc = exact_range_guard(h, nq, queries, row_stride, radius, lims, total);
    if (rc)
        return rc;
    SlotsArg sl;
    if ((rc = exact_values_guard(h, "exact_range_search_values", &sl)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, lims, nullptr, total);
    const size_t d = (h->parent ? h->parent : h)->base_d;
    if ((rc = h->ex_raw.ensure(nq * d)) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))) ||
        (rc = h->bs_qslots.ensure(nq * 2 * sizeof(uint32_t))))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d, queries, row_stride, d, nq, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, query_ranges, nq * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    sl.d_ranges = h->bs_qslots.as<uint32_t>();
    if ((rc = exact_range_dev(h, nq, h->ex_raw.as<uint8_t>(), d, radius, h->xr_lims.as<uint64_t>(), total, sl)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}
