#include "capi_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// The float16 base store: float-valued corpora (DEEP1B: 96-d float) kept as halves in HBM, with the exact
// search on the f16 matrix cores that writes their ground truth (kernels_exact_f16.hip).  The re-rank against it is
// capi_rerank.cpp's, which serves whichever store the handle holds.

namespace {

// Pieces of at most 512 MB of float32 rows on their way through the device staging buffer.  A host chunk of one piece --
// upload_base_fvecs' default chunks are -- crosses the bus once and serves both passes from the buffer; a larger chunk is
// copied twice, once per pass, because the whole chunk is checked before any of it is written.
size_t stage_rows(size_t d) { return std::max<size_t>(1, ((size_t)512 << 20) / (d * sizeof(float))); }

// rows [r0, r0 + m) of host `rows` packed into the staging buffer, on the handle's stream
int stage_piece(ivfhnsw_gpu *h, const float *rows, size_t row_stride, size_t d, size_t r0, size_t m)
{
    HIP_TRY(hipMemcpy2DAsync(h->base_stage.p, d * sizeof(float), rows + r0 * row_stride, row_stride * sizeof(float),
                             d * sizeof(float), m, hipMemcpyHostToDevice, h->stream));
    return IVFHNSW_OK;
}

// rows [first, first + count) of the store from float32 `rows` at row_stride floats (device memory when on_device).  The
// whole chunk is checked before anything changes: a value that is NaN or does not round to a finite half refuses the call
// with the store -- on first == 0 the previous one -- as it was.
int upload_base_f16_impl(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const float *rows, size_t row_stride,
                         bool on_device)
{
    const char *who = on_device ? "upload_base_f16_dev" : "upload_base_f16";
    int rc = table_change_guard(h, kUploads, who, false);
    if (rc)
        return rc;
    if (n == 0)
        return base_store_free(h);
    if ((rc = base_store_args(n, d, 256, first, count, rows, row_stride)))
        return rc;
    if (on_device && ((uintptr_t)rows & 3))
        return fail(IVFHNSW_ERR_INVALID, "%s: rows must be 4-byte aligned", who);
    const size_t piece = stage_rows(d);
    const bool one_piece = count <= piece; // a host chunk of one piece is staged once for both passes
    if (count) {
        if (!on_device && (rc = h->base_stage.ensure(std::min(piece, count) * d * sizeof(float))))
            return rc;
        if ((rc = h->base_flag.ensure(sizeof(uint32_t))))
            return rc;
        uint32_t bad = 0, *flag = h->base_flag.as<uint32_t>();
        HIP_TRY(hipMemsetAsync(flag, 0, sizeof(uint32_t), h->stream));
        if (on_device)
            HIP_TRY(launch_f16_check(h->stream, rows, row_stride, count, (int)d, flag));
        for (size_t r0 = 0; !on_device && r0 < count; r0 += piece) {
            const size_t m = std::min(piece, count - r0);
            if ((rc = stage_piece(h, rows, row_stride, d, r0, m)))
                return rc;
            HIP_TRY(launch_f16_check(h->stream, h->base_stage.as<float>(), d, m, (int)d, flag));
        }
        HIP_TRY(hipMemcpyAsync(&bad, flag, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (bad)
            return fail(IVFHNSW_ERR_INVALID, "%s: rows [%zu, %zu) hold a NaN or a value that does not round to a finite half", who,
                        first, first + count);
    }
    if ((rc = base_store_open(h, IVFHNSW_BASE_F16, who, n, d, first)))
        return rc;
    unsigned char *dst = h->base_rows.as<unsigned char>() + first * d * 2;
    float *norms = h->base_norms.as<float>() + first;
    if (on_device) {
        HIP_TRY(launch_f16_store(h->stream, rows, row_stride, dst, norms, count, (int)d));
    } else {
        for (size_t r0 = 0; r0 < count; r0 += piece) {
            const size_t m = std::min(piece, count - r0);
            if (!one_piece && (rc = stage_piece(h, rows, row_stride, d, r0, m)))
                return rc;
            HIP_TRY(launch_f16_store(h->stream, h->base_stage.as<float>(), d, dst + r0 * d * 2, norms + r0, m, (int)d));
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// Splits of a call.  The sweep's workgroups hold 64 to 100 KB of LDS, so one or two are resident per CU and a grid that is
// a little larger than what is resident runs a second, nearly empty round: with s splits the call takes
// ceil(row_blocks * s / resident) rounds of 1 / s of the columns each.  The fewest splits within 5 % of the best such
// product (every split warms its thresholds up anew, and the merge reads them all); a split never shorter than 4096
// columns.  256 CUs, as sweep_splits_for counts them, and 160 KB of LDS each; what a workgroup holds is
// exact_f16_lds_bytes', the one place that knows the kernel's CAP and WAVES per k, so this rule follows any change of
// them as long as that function does.  Above k = 32 the sweep is bound by the selection, whose warm-up every
// split repeats, not by the rounds: there the rule of the uint8 sweep stays (measured).
// The rule itself takes the kernel's shape -- rpb query rows and lds bytes per workgroup -- so that the range sweep
// (DESIGN.md 3.28), whose workgroups hold the two tiles only, is cut by the same rule with its own numbers.  More than two
// workgroups per CU are not counted on for either kernel: whether they help has not been measured.
int f16_splits_rule(size_t nq, size_t nx, size_t rpb, size_t lds)
{
    const size_t row_blocks = (nq + rpb - 1) / rpb;
    const size_t per_cu = std::max<size_t>(1, std::min<size_t>(2, ((size_t)160 << 10) / lds));
    const size_t resident = 256 * per_cu, max_s = std::min<size_t>(64, std::max<size_t>(1, (nx + 4095) / 4096));
    auto cost = [&](size_t s) { return (double)((row_blocks * s + resident - 1) / resident) / (double)s; };
    double best = cost(1);
    for (size_t s = 2; s <= max_s; s++)
        best = std::min(best, cost(s));
    for (size_t s = 1; s <= max_s; s++)
        if (cost(s) <= 1.05 * best)
            return (int)s;
    return 1;
}

int exact_f16_splits_for(size_t nq, size_t nx, size_t d, int k)
{
    if (k > 32)
        return exact_splits_for(nq, nx, k);
    return f16_splits_rule(nq, nx, (size_t)exact_rows_per_block(k), exact_f16_lds_bytes((int)d, k));
}

int exact_range_f16_splits_for(size_t nq, size_t nx, size_t d) { return f16_splits_rule(nq, nx, 128, exact_range_f16_lds_bytes((int)d)); }

// what every exact call on the half store checks first: the handle; the store (*b: a view searches its parent's), its
// kind, and that the holder has no base filter or slots installed (neither can be, on a half store: the check stands for
// the day one can).  Base tags can and base values can (3.31); the calls that do not name them ignore
// them as the uint8 store's do.
int exact_f16_guard(ivfhnsw_gpu *h, const char *who, const char *u8_call, const ivfhnsw_gpu **b)
{
    int rc = bind(h);
    if (rc)
        return rc;
    *b = h->parent ? h->parent : h;
    if (!(*b)->base_n)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_base_f16", who);
    if ((*b)->base_kind != IVFHNSW_BASE_F16)
        return fail(IVFHNSW_ERR_STATE, "%s on a uint8 store: %s serves it", who, u8_call);
    const bool slot_set = std::any_of(std::begin((*b)->bslots), std::end((*b)->bslots), [](const BaseSlot &s) { return s.mode >= 0; });
    if ((*b)->bf_mode >= 0 || slot_set)
        return fail(IVFHNSW_ERR_STATE, "%s: the holder has a base filter or slots installed, which it does not take", who);
    return IVFHNSW_OK;
}

// The splits of a _tags call's two launches, for a chunk of m queries on a store of n rows.  Dense: the
// plain call's rule fed with the most rows the Dense launch can have, the chunk's queries padded to a strip -- not with the
// rows of every strip the plan can have, most of which are other tags': an all-NONE batch is then cut as the plain call
// is.  Indirect: the uint8 sweep's rule (its workgroups hold the candidate buffers only, as that sweep's do) over the rows
// of every strip and the columns of the longest row list; a shorter list cuts its own columns and leaves the splits it
// does not reach empty.
void exact_f16_tag_splits(const ivfhnsw_gpu *b, size_t m, int k, int *ns_dense, int *ns_ind)
{
    *ns_dense = exact_f16_splits_for((m + 31) / 32 * 32, b->base_n, b->base_d, k);
    *ns_ind = b->bt_tagged ? exact_splits_for(sweep_tag_strip_bound(m, b->bt_in_use) * 32, b->bt_max_rows, k) : 1;
}

// as exact_impl of the uint8 store (capi_exact.cpp) without a column map: the chunks, the splits and the staging of a host call
int exact_f16_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k, float *distances, int64_t *labels,
                   bool on_device)
{
    const char *who = on_device ? "exact_search_f16_dev" : "exact_search_f16";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "exact_search", &b);
    if (rc)
        return rc;
    if (k < 1 || k > 100)
        return fail(IVFHNSW_ERR_INVALID, "%s needs 1 <= k <= 100 (k %zu)", who, k);
    if (nq == 0)
        return IVFHNSW_OK;
    const size_t d = b->base_d, n = b->base_n;
    if (!queries || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "%s: null query/result buffer", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (on_device && ((uintptr_t)queries & 3))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries must be 4-byte aligned", who);

    const int nsplit = h->opt_exact_splits > 0 ? h->opt_exact_splits : exact_f16_splits_for(std::min(nq, kExactChunk), n, d, (int)k);
    size_t chunk = kExactPartBytes / ((size_t)nsplit * k * sizeof(uint64_t));
    chunk = std::min(nq, std::max<size_t>(128, std::min(kExactChunk, chunk / 128 * 128)));
    if ((rc = h->ex_q.ensure(chunk * d * 2)) || (rc = h->ex_qn.ensure(chunk * sizeof(float))) ||
        (rc = h->ex_part.ensure((size_t)nsplit * chunk * k * sizeof(uint64_t))))
        return rc;
    if (!on_device && ((rc = h->ex_raw.ensure(chunk * d * sizeof(float))) || (rc = h->ex_dist.ensure(chunk * k * sizeof(float))) ||
                       (rc = h->ex_lab.ensure(chunk * k * sizeof(int64_t)))))
        return rc;
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const size_t m = std::min(chunk, nq - q0);
        const float *src = queries + q0 * row_stride;
        size_t src_stride = row_stride;
        if (!on_device) {
            HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), src, row_stride * sizeof(float), d * sizeof(float), m,
                                     hipMemcpyHostToDevice, h->stream));
            src = h->ex_raw.as<float>();
            src_stride = d;
        }
        float *od = on_device ? distances + q0 * k : h->ex_dist.as<float>();
        int64_t *ol = on_device ? labels + q0 * k : h->ex_lab.as<int64_t>();
        // the queries rounded, permuted and normed as the store's rows were
        HIP_TRY(launch_f16_store(h->stream, src, src_stride, h->ex_q.p, h->ex_qn.as<float>(), m, (int)d));
        HIP_TRY(launch_exact_search_f16(h->stream, h->ex_q.p, h->ex_qn.as<float>(), b->base_rows.p, b->base_norms.as<float>(), m, n,
                                        (int)d, (int)k, nsplit, h->ex_part.as<unsigned long long>(), od, ol));
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(distances + q0 * k, od, m * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(labels + q0 * k, ol, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            // the next chunk reuses the pageable source and the staging buffers
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return IVFHNSW_OK;
}

// With a base tag per query: exact_impl's _tags path (capi_exact.cpp, 3.22) around the half store's two
// kernels.  Per chunk: the tag plan (launch_tag_strip_plan, which never looks at the rows' type), the queries rounded,
// permuted and normed into the plan's strip order in one pass, the Dense strips by the staged kernel and the Indirect ones
// by the per-wave kernel, each under its own split count, and the merge that scatters every strip row to its query.
int exact_f16_tags_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k, const uint16_t *query_tags,
                        float *distances, int64_t *labels, bool on_device)
{
    if (!query_tags)
        return exact_f16_impl(h, nq, queries, row_stride, k, distances, labels, on_device);
    const char *who = on_device ? "exact_search_f16_tags_dev" : "exact_search_f16_tags";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "exact_search_tags", &b);
    if (rc)
        return rc;
    if (k < 1 || k > 100)
        return fail(IVFHNSW_ERR_INVALID, "%s needs 1 <= k <= 100 (k %zu)", who, k);
    if (nq == 0)
        return IVFHNSW_OK;
    const size_t d = b->base_d, n = b->base_n;
    if (!queries || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "%s: null query/result buffer", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (on_device && (((uintptr_t)queries & 3) || ((uintptr_t)query_tags & 1)))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries must be 4-byte and query tags 2-byte aligned", who);
    TagRows tr;
    size_t in_use = 0;
    if ((rc = base_tags_call(b, who, &tr, &in_use)))
        return rc;
    const unsigned forms = 1u << kSweepColsDense | (b->bt_tagged ? 1u << kSweepColsIndirect : 0u);

    int ns_dense, ns_ind;
    exact_f16_tag_splits(b, std::min(nq, kExactChunk), (int)k, &ns_dense, &ns_ind);
    if (h->opt_exact_splits > 0)
        ns_dense = ns_ind = h->opt_exact_splits;
    const int nsplit = std::max(ns_dense, ns_ind);
    // with many tags the padded rows, not the queries, size the partial tables
    const size_t chunk = std::min(nq, sweep_tag_chunk(nsplit, k, in_use));
    const size_t bound = sweep_tag_strip_bound(chunk, in_use), rows = bound * 32;
    if ((rc = h->ex_q.ensure(rows * d * 2)) || (rc = h->ex_qn.ensure(rows * sizeof(float))) ||
        (rc = h->ex_part.ensure((size_t)nsplit * rows * k * sizeof(uint64_t))) || (rc = h->bs_plan.ensure(sweep_tag_plan_bytes(bound))) ||
        (rc = h->bt_work.ensure(tag_plan_work_words(chunk) * sizeof(uint32_t))))
        return rc;
    if (!on_device && ((rc = h->ex_raw.ensure(chunk * d * sizeof(float))) || (rc = h->bs_qslots.ensure(chunk * sizeof(uint16_t))) ||
                       (rc = h->ex_dist.ensure(chunk * k * sizeof(float))) || (rc = h->ex_lab.ensure(chunk * k * sizeof(int64_t)))))
        return rc;
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const size_t m = std::min(chunk, nq - q0);
        const float *src = queries + q0 * row_stride;
        const uint16_t *dt = query_tags + q0;
        size_t src_stride = row_stride;
        if (!on_device) {
            HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), src, row_stride * sizeof(float), d * sizeof(float), m,
                                     hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, dt, m * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
            src = h->ex_raw.as<float>();
            src_stride = d;
            dt = h->bs_qslots.as<uint16_t>();
        }
        float *od = on_device ? distances + q0 * k : h->ex_dist.as<float>();
        int64_t *ol = on_device ? labels + q0 * k : h->ex_lab.as<int64_t>();
        StripPlan sp;
        {
            StageScope sc(h, IVFHNSW_STAGE_PLAN); // the plan and the gather, accounted apart from the sweep
            HIP_TRY(launch_tag_strip_plan(h->stream, dt, m, tr, h->bs_plan.p, bound, h->bt_work.as<uint32_t>(), &sp));
            // the queries as the store holds its rows, in strip order; a padding row repeats the chunk's first query
            HIP_TRY(launch_f16_store_rows(h->stream, src, src_stride, h->ex_q.p, h->ex_qn.as<float>(), rows, (int)d, sp.strip_rows));
        }
        HIP_TRY(launch_exact_search_f16_strips(h->stream, h->ex_q.p, h->ex_qn.as<float>(), b->base_rows.p, b->base_norms.as<float>(), m,
                                               bound, n, (int)d, (int)k, ns_dense, ns_ind, h->ex_part.as<unsigned long long>(), od, ol, sp,
                                               forms));
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(distances + q0 * k, od, m * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(labels + q0 * k, ol, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            // the next chunk reuses the pageable source and the staging buffers
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return IVFHNSW_OK;
}

// The splits of a _values call's two launches, for a chunk of m queries on a store of n rows.  Dense: as
// under tags, the plain call's rule over the chunk's queries padded to a strip.  Windowed: the uint8 sweep's rule (the
// windowed kernel's workgroups hold the candidate buffers only) over the padded rows of every strip the plan can have and
// the rows of the store, which is the longest span a strip can have; a shorter span cuts its own columns.  A first rule:
// it has not been measured against its neighbours.
void exact_f16_value_splits(const ivfhnsw_gpu *b, size_t m, int k, int *ns_dense, int *ns_win)
{
    *ns_dense = exact_f16_splits_for((m + 31) / 32 * 32, b->base_n, b->base_d, k);
    *ns_win = b->bv_vals.p ? exact_splits_for(sweep_value_strip_bound(m) * 32, b->base_n, k) : 1;
}

// With an interval of base values per query: exact_impl's _values path (capi_exact.cpp, 3.25) around the
// half store's kernels, shaped as exact_f16_tags_impl.  Per chunk (sweep_value_chunk): the value plan
// (launch_value_strip_plan, which never looks at the rows' type) with the window of every strip row, the queries rounded,
// permuted and normed into strip order, the Dense strips -- the queries whose window is the whole store -- by the staged
// kernel and the windowed ones by exact_f16_windows_kernel, each under its own split count, and the merge.
int exact_f16_values_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k, const uint32_t *query_ranges,
                          float *distances, int64_t *labels, bool on_device)
{
    if (!query_ranges)
        return exact_f16_impl(h, nq, queries, row_stride, k, distances, labels, on_device);
    const char *who = on_device ? "exact_search_f16_values_dev" : "exact_search_f16_values";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "exact_search_values", &b);
    if (rc)
        return rc;
    if (k < 1 || k > 100)
        return fail(IVFHNSW_ERR_INVALID, "%s needs 1 <= k <= 100 (k %zu)", who, k);
    if (nq == 0)
        return IVFHNSW_OK;
    const size_t d = b->base_d, n = b->base_n;
    if (!queries || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "%s: null query/result buffer", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (on_device && (((uintptr_t)queries & 3) || ((uintptr_t)query_ranges & 7)))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries must be 4-byte and query ranges 8-byte aligned", who);
    ValueRows vr;
    if ((rc = base_values_call(b, who, &vr)))
        return rc;
    // the windowed sweep only where a row holds a value
    const unsigned forms = 1u << kSweepColsDense | (vr.vals ? 1u << kSweepColsIndirect : 0u);

    int ns_dense, ns_win;
    exact_f16_value_splits(b, std::min(nq, kExactChunk), (int)k, &ns_dense, &ns_win);
    if (h->opt_exact_splits > 0)
        ns_dense = ns_win = h->opt_exact_splits;
    const int nsplit = std::max(ns_dense, ns_win);
    const size_t chunk = std::min(nq, sweep_value_chunk(nsplit, k));
    const size_t bound = sweep_value_strip_bound(chunk), rows = bound * 32;
    if ((rc = h->ex_q.ensure(rows * d * 2)) || (rc = h->ex_qn.ensure(rows * sizeof(float))) ||
        (rc = h->ex_part.ensure((size_t)nsplit * rows * k * sizeof(uint64_t))) || (rc = h->bs_plan.ensure(sweep_value_plan_bytes(bound))) ||
        (rc = h->bv_work.ensure(value_plan_work_words(chunk) * sizeof(uint32_t))))
        return rc;
    if (!on_device && ((rc = h->ex_raw.ensure(chunk * d * sizeof(float))) || (rc = h->bs_qslots.ensure(chunk * 2 * sizeof(uint32_t))) ||
                       (rc = h->ex_dist.ensure(chunk * k * sizeof(float))) || (rc = h->ex_lab.ensure(chunk * k * sizeof(int64_t)))))
        return rc;
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const size_t m = std::min(chunk, nq - q0);
        const float *src = queries + q0 * row_stride;
        const uint32_t *dr = query_ranges + 2 * q0;
        size_t src_stride = row_stride;
        if (!on_device) {
            HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), src, row_stride * sizeof(float), d * sizeof(float), m,
                                     hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, dr, m * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            src = h->ex_raw.as<float>();
            src_stride = d;
            dr = h->bs_qslots.as<uint32_t>();
        }
        float *od = on_device ? distances + q0 * k : h->ex_dist.as<float>();
        int64_t *ol = on_device ? labels + q0 * k : h->ex_lab.as<int64_t>();
        StripPlan sp;
        const StripWin *win = nullptr;
        {
            StageScope sc(h, IVFHNSW_STAGE_PLAN); // the plan and the gather, accounted apart from the sweep
            HIP_TRY(launch_value_strip_plan(h->stream, dr, m, vr, h->bs_plan.p, bound, h->bv_work.as<uint32_t>(), &sp, &win));
            // the queries as the store holds its rows, in strip order; a padding row repeats the chunk's first query
            HIP_TRY(launch_f16_store_rows(h->stream, src, src_stride, h->ex_q.p, h->ex_qn.as<float>(), rows, (int)d, sp.strip_rows));
        }
        HIP_TRY(launch_exact_search_f16_strips(h->stream, h->ex_q.p, h->ex_qn.as<float>(), b->base_rows.p, b->base_norms.as<float>(), m,
                                               bound, n, (int)d, (int)k, ns_dense, ns_win, h->ex_part.as<unsigned long long>(), od, ol, sp,
                                               forms, win));
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(distances + q0 * k, od, m * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(labels + q0 * k, ol, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            // the next chunk reuses the pageable source and the staging buffers
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return IVFHNSW_OK;
}

// Queries per pass of a _tags_values k-search: as sweep_tag_chunk, the partial tables over the padded rows of BOTH plans.
// At 128 it always fits (64 * (132 + 6) * 32 * 100 * 8 = 226 MB).
size_t exact_f16_tags_values_chunk(int nsplit, size_t k, size_t tags_in_use)
{
    const size_t per_strip = (size_t)nsplit * 32 * k * sizeof(uint64_t);
    size_t chunk = kExactChunk;
    while (chunk > 128 && per_strip * (sweep_tag_strip_bound(chunk, tags_in_use) + sweep_value_strip_bound(chunk)) > kExactPartBytes)
        chunk -= 128;
    return chunk;
}

// With a base tag AND an interval of base values per query.  Per chunk the queries are parted on the
// device by tag == NONE, without moving them: one small kernel writes the value plan's intervals -- a tagged query's is
// empty, so it gets no strip there -- and the tag plan's minor keys, a tagged query's lo.  The untagged side is the _values
// call's: the value plan, its Dense strips by the staged kernel and its windowed ones by exact_f16_windows_kernel.  The
// tagged side is the tag plan, a tag's queries ordered by lo, whose Indirect strips go to exact_f16_gated_kernel (its Dense
// strips, the untagged queries, are swept by nobody).  Each sweep under its own split count; one merge scatters every
// strip row of both plans to its query's place.  The host form knows the chunk's tags and plans and launches only the sides
// that have queries; the device form launches both -- the workgroups of a side without strips leave at once.
int exact_f16_tags_values_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k, const uint16_t *query_tags,
                               const uint32_t *query_ranges, float *distances, int64_t *labels, bool on_device)
{
    if (!query_ranges)
        return exact_f16_tags_impl(h, nq, queries, row_stride, k, query_tags, distances, labels, on_device);
    if (!query_tags)
        return exact_f16_values_impl(h, nq, queries, row_stride, k, query_ranges, distances, labels, on_device);
    const char *who = on_device ? "exact_search_f16_tags_values_dev" : "exact_search_f16_tags_values";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "no call", &b); // (the uint8 store has no counterpart)
    if (rc)
        return rc;
    if (k < 1 || k > 100)
        return fail(IVFHNSW_ERR_INVALID, "%s needs 1 <= k <= 100 (k %zu)", who, k);
    if (nq == 0)
        return IVFHNSW_OK;
    const size_t d = b->base_d, n = b->base_n;
    if (!queries || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "%s: null query/result buffer", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (on_device && (((uintptr_t)queries & 3) || ((uintptr_t)query_tags & 1) || ((uintptr_t)query_ranges & 3)))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries and query ranges must be 4-byte and query tags 2-byte aligned", who);
    TagRows tr;
    ValueRows vr;
    size_t in_use = 0;
    if ((rc = base_tags_call(b, who, &tr, &in_use)) || (rc = base_values_call(b, who, &vr)))
        return rc;

    int ns_dense, ns_win, ns_tag; // (both rules cut the Dense strips alike)
    exact_f16_value_splits(b, std::min(nq, kExactChunk), (int)k, &ns_dense, &ns_win);
    exact_f16_tag_splits(b, std::min(nq, kExactChunk), (int)k, &ns_dense, &ns_tag);
    if (h->opt_exact_splits > 0)
        ns_dense = ns_win = ns_tag = h->opt_exact_splits;
    const int nsplit = std::max(ns_dense, std::max(ns_win, ns_tag));
    const size_t chunk = std::min(nq, exact_f16_tags_values_chunk(nsplit, k, in_use));
    const size_t bound_v = sweep_value_strip_bound(chunk), bound_t = sweep_tag_strip_bound(chunk, in_use);
    const size_t rows_v = bound_v * 32, rows = (bound_v + bound_t) * 32;
    const size_t plan_v = (sweep_value_plan_bytes(bound_v) + 15) & ~(size_t)15, vwork = value_plan_work_words(chunk);
    // behind the value plan's work words: the tag plan's minor keys [chunk] and the value plan's intervals [2 chunk]
    if ((rc = h->ex_q.ensure(rows * d * 2)) || (rc = h->ex_qn.ensure(rows * sizeof(float))) ||
        (rc = h->ex_part.ensure((size_t)nsplit * rows * k * sizeof(uint64_t))) ||
        (rc = h->bs_plan.ensure(plan_v + sweep_tag_plan_bytes(bound_t))) ||
        (rc = h->bt_work.ensure(tag_plan_work_words(chunk) * sizeof(uint32_t))) ||
        (rc = h->bv_work.ensure((vwork + 3 * chunk) * sizeof(uint32_t))))
        return rc;
    // the host form stages a chunk's intervals and, behind them, its tags
    if (!on_device && ((rc = h->ex_raw.ensure(chunk * d * sizeof(float))) ||
                       (rc = h->bs_qslots.ensure(chunk * (2 * sizeof(uint32_t) + sizeof(uint16_t)))) ||
                       (rc = h->ex_dist.ensure(chunk * k * sizeof(float))) || (rc = h->ex_lab.ensure(chunk * k * sizeof(int64_t)))))
        return rc;
    uint32_t *lo_keys = h->bv_work.as<uint32_t>() + vwork, *vranges = lo_keys + chunk;
    for (size_t q0 = 0; q0 < nq; q0 += chunk) {
        const size_t m = std::min(chunk, nq - q0);
        const float *src = queries + q0 * row_stride;
        const uint16_t *dt = query_tags + q0;
        const uint32_t *dr = query_ranges + 2 * q0;
        size_t src_stride = row_stride;
        bool side_v = true, side_t = b->bt_tagged; // (a holder without tagged rows has no row list to sweep)
        if (!on_device) {
            side_v = std::any_of(dt, dt + m, [](uint16_t t) { return t == kTagNone; });
            side_t = side_t && std::any_of(dt, dt + m, [](uint16_t t) { return t != kTagNone; });
            uint32_t *sr = h->bs_qslots.as<uint32_t>();
            uint16_t *st = reinterpret_cast<uint16_t *>(sr + 2 * chunk);
            HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), src, row_stride * sizeof(float), d * sizeof(float), m,
                                     hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(sr, dr, m * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(st, dt, m * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
            src = h->ex_raw.as<float>();
            src_stride = d;
            dr = sr;
            dt = st;
        }
        float *od = on_device ? distances + q0 * k : h->ex_dist.as<float>();
        int64_t *ol = on_device ? labels + q0 * k : h->ex_lab.as<int64_t>();
        StripPlan spv, spt;
        const StripWin *win = nullptr;
        unsigned char *qh = h->ex_q.as<unsigned char>();
        {
            StageScope sc(h, IVFHNSW_STAGE_PLAN); // the plans and the gathers, accounted apart from the sweeps
            HIP_TRY(launch_f16_tags_values_split(h->stream, dt, dr, m, lo_keys, vranges));
            // the queries as the store holds its rows, in each plan's strip order; a padding row repeats the chunk's first query
            if (side_v) {
                HIP_TRY(launch_value_strip_plan(h->stream, vranges, m, vr, h->bs_plan.p, bound_v, h->bv_work.as<uint32_t>(), &spv, &win));
                HIP_TRY(launch_f16_store_rows(h->stream, src, src_stride, qh, h->ex_qn.as<float>(), rows_v, (int)d, spv.strip_rows));
            }
            if (side_t) {
                HIP_TRY(launch_tag_strip_plan(h->stream, dt, m, tr, h->bs_plan.as<unsigned char>() + plan_v, bound_t, h->bt_work.as<uint32_t>(),
                                              &spt, lo_keys));
                HIP_TRY(launch_f16_store_rows(h->stream, src, src_stride, qh + rows_v * d * 2, h->ex_qn.as<float>() + rows_v, bound_t * 32,
                                              (int)d, spt.strip_rows));
            }
        }
        HIP_TRY(launch_exact_search_f16_tags_values(h->stream, qh, h->ex_qn.as<float>(), b->base_rows.p, b->base_norms.as<float>(), m, bound_v,
                                                    bound_t, n, (int)d, (int)k, ns_dense, ns_win, ns_tag, h->ex_part.as<unsigned long long>(), od,
                                                    ol, side_v ? &spv : nullptr, win, vr.vals != nullptr, side_t ? &spt : nullptr, dt, dr,
                                                    vr.vals));
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
// Exact range search of the half store: the sequence of the uint8 call (capi_exact.cpp, 3.17) -- count ->
// prefix -> (one synchronisation: the host sizes the results) -> fill -- around exact_range_f16_kernel.

// one form of the sweep over every chunk of the call's queries (h->ex_q, h->ex_qn: all of them, as the store holds rows)
int exact_range_f16_pass(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, bool fill, size_t nq, float radius, int nsplit, int map_shift,
                         float *dist, int64_t *labels, size_t out_cap)
{
    const size_t d = b->base_d;
    StageScope sc(h, fill ? IVFHNSW_STAGE_SELECT : IVFHNSW_STAGE_SCAN); // accounted as exact_range_search accounts its passes
    uint32_t *map = h->opt_exact_range_map ? h->xr_map.as<uint32_t>() : nullptr;
    for (size_t q0 = 0; q0 < nq; q0 += kExactChunk) // (kExactChunk % 128 == 0: a chunk starts a workgroup's strip)
        HIP_TRY(launch_exact_range_f16(h->stream, fill, h->ex_q.as<unsigned char>() + q0 * d * 2, h->ex_qn.as<float>() + q0,
                                       b->base_rows.p, b->base_norms.as<float>(), std::min(kExactChunk, nq - q0), q0, b->base_n, (int)d,
                                       radius, nsplit, h->xr_slices.as<uint32_t>(), h->xr_tot.as<unsigned long long>(), map, map_shift,
                                       dist, labels, out_cap));
    return IVFHNSW_OK;
}

// device pointers, the arguments checked (nq > 0)
int exact_range_f16_dev(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const char *who, size_t nq, const float *d_queries, size_t row_stride,
                        float radius, uint64_t *d_lims, uint64_t *total)
{
    const size_t d = b->base_d, n = b->base_n;
    const int nsplit = h->opt_exact_splits > 0 ? h->opt_exact_splits : exact_range_f16_splits_for(std::min(nq, kExactChunk), n, d);
    const size_t len = nq * (size_t)nsplit + 1;
    size_t map_bytes = 0;
    const int map_shift = exact_range_map_shift(nq, n, 2 * d, nsplit, &map_bytes);
    int rc;
    if ((rc = h->ex_q.ensure(nq * d * 2)) || (rc = h->ex_qn.ensure(nq * sizeof(float))) ||
        (rc = h->xr_slices.ensure(len * sizeof(uint32_t))) || (rc = h->xr_part.ensure(append_scan_parts(len) * sizeof(uint32_t))) ||
        (rc = h->xr_tot.ensure(sizeof(unsigned long long))) || (h->opt_exact_range_map && (rc = h->xr_map.ensure(map_bytes))))
        return rc;
    // every query of the call rounded, permuted and normed as the store's rows were, once for both passes
    HIP_TRY(launch_f16_store(h->stream, d_queries, row_stride, h->ex_q.p, h->ex_qn.as<float>(), nq, (int)d));
    HIP_TRY(hipMemsetAsync(h->xr_slices.p, 0, len * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->xr_tot.p, 0, sizeof(unsigned long long), h->stream));
    if ((rc = exact_range_f16_pass(h, b, false, nq, radius, nsplit, map_shift, nullptr, nullptr, 0)))
        return rc;
    unsigned long long tot = 0;
    if ((rc = exact_range_total(h, who, len, &tot)))
        return rc;
    RangeOut out;
    if ((rc = out.reserve(h, tot)))
        return rc;
    HIP_TRY(launch_range_lims(h->stream, h->xr_slices.as<uint32_t>(), (int)nq, nsplit, d_lims));
    if (tot && (rc = exact_range_f16_pass(h, b, true, nq, radius, nsplit, map_shift, out.dist(h), out.lab(h), (size_t)tot)))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    out.commit(h, tot);
    *total = tot;
    return IVFHNSW_OK;
}

int exact_range_f16_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, float radius, uint64_t *lims,
                         uint64_t *total, bool on_device)
{
    const char *who = on_device ? "exact_range_search_f16_dev" : "exact_range_search_f16";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "exact_range_search", &b);
    if (rc)
        return rc;
    if (std::isnan(radius))
        return fail(IVFHNSW_ERR_INVALID, "%s: the radius is NaN", who);
    if (nq == 0)
        return exact_range_none(h, on_device ? nullptr : lims, on_device ? lims : nullptr, total);
    const size_t d = b->base_d;
    if (!queries || !lims || !total)
        return fail(IVFHNSW_ERR_INVALID, "%s: null queries, lims or total", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (nq > kMaxBatchAll)
        return fail(IVFHNSW_ERR_INVALID, "%s is limited to %zu queries per call", who, kMaxBatchAll);
    if (on_device && (((uintptr_t)queries & 3) || ((uintptr_t)lims & 7)))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries must be 4-byte and lims 8-byte aligned", who);
    if (on_device)
        return exact_range_f16_dev(h, b, who, nq, queries, row_stride, radius, lims, total);
    if ((rc = h->ex_raw.ensure(nq * d * sizeof(float))) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), queries, row_stride * sizeof(float), d * sizeof(float), nq,
                             hipMemcpyHostToDevice, h->stream));
    if ((rc = exact_range_f16_dev(h, b, who, nq, h->ex_raw.as<float>(), d, radius, h->xr_lims.as<uint64_t>(), total)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// ... with a base tag per query: the same sequence around the two kernels a tag plan takes, the way
// exact_range_dev of the uint8 store carries its RangeStrips.  Per chunk of kExactChunk queries the tag plan is made once
// and kept for both passes, chunk i's gathered queries at row i * bound * 32 of h->ex_q / h->ex_qn and its strips from
// strip i * bound of the tile map.
struct F16RangeStrips {
    size_t bound = 0;
    unsigned forms = 0;
    int ns_dense = 1, ns_ind = 1;
    std::vector<StripPlan> plans;
    std::vector<const StripWin *> wins; // a _values call (3.32): the windows of each plan's strip rows; else empty
};

int exact_range_f16_strips_pass(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const F16RangeStrips &rs, bool fill, size_t nq, float radius,
                                int map_shift, float *dist, int64_t *labels, size_t out_cap)
{
    const size_t d = b->base_d, rows = rs.bound * 32;
    StageScope sc(h, fill ? IVFHNSW_STAGE_SELECT : IVFHNSW_STAGE_SCAN);
    uint32_t *map = h->opt_exact_range_map ? h->xr_map.as<uint32_t>() : nullptr;
    for (size_t q0 = 0, i = 0; q0 < nq; q0 += kExactChunk, i++)
        HIP_TRY(launch_exact_range_f16_strips(h->stream, fill, h->ex_q.as<unsigned char>() + i * rows * d * 2, h->ex_qn.as<float>() + i * rows,
                                              b->base_rows.p, b->base_norms.as<float>(), rs.bound, q0, b->base_n, (int)d, radius, rs.ns_dense,
                                              rs.ns_ind, h->xr_slices.as<uint32_t>(), h->xr_tot.as<unsigned long long>(), map, map_shift,
                                              dist, labels, out_cap, rs.plans[i], rs.forms, rs.wins.empty() ? nullptr : rs.wins[i]));
    return IVFHNSW_OK;
}

// device pointers, the arguments checked (nq > 0)
int exact_range_f16_tags_dev(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const char *who, size_t nq, const float *d_queries, size_t row_stride,
                             const uint16_t *d_tags, const TagRows &tr, size_t in_use, float radius, uint64_t *d_lims, uint64_t *total)
{
    const size_t d = b->base_d, n = b->base_n, first = std::min(nq, kExactChunk), nchunks = (nq + kExactChunk - 1) / kExactChunk;
    F16RangeStrips rs;
    rs.bound = sweep_tag_strip_bound(first, in_use);
    rs.forms = 1u << kSweepColsDense | (b->bt_tagged ? 1u << kSweepColsIndirect : 0u);
    // Dense: the plain call's rule over the chunk's queries padded to a strip; Indirect: the uint8 sweep's rule (k = 1: a
    // workgroup of four strips) over the rows of every strip and the longest row list
    rs.ns_dense = exact_range_f16_splits_for((first + 31) / 32 * 32, n, d);
    rs.ns_ind = b->bt_tagged ? exact_splits_for(rs.bound * 32, b->bt_max_rows, 1) : 1;
    if (h->opt_exact_splits > 0)
        rs.ns_dense = rs.ns_ind = h->opt_exact_splits;
    rs.plans.resize(nchunks);
    const int nsplit = std::max(rs.ns_dense, rs.ns_ind); // the one width of the slices table
    const size_t len = nq * (size_t)nsplit + 1, rows = nchunks * rs.bound * 32, plan_bytes = sweep_tag_plan_bytes(rs.bound);
    size_t map_bytes = 0;
    const int map_shift = exact_range_map_shift(rows, n, 2 * d, nsplit, &map_bytes);
    map_bytes = rows / 32 * exact_range_f16_strips_map_words(n, rs.ns_dense, rs.ns_ind, map_shift) * sizeof(uint32_t);
    int rc;
    if ((rc = h->ex_q.ensure(rows * d * 2)) || (rc = h->ex_qn.ensure(rows * sizeof(float))) ||
        (rc = h->xr_slices.ensure(len * sizeof(uint32_t))) || (rc = h->xr_part.ensure(append_scan_parts(len) * sizeof(uint32_t))) ||
        (rc = h->xr_tot.ensure(sizeof(unsigned long long))) || (h->opt_exact_range_map && (rc = h->xr_map.ensure(map_bytes))) ||
        (rc = h->bs_plan.ensure(nchunks * plan_bytes)) || (rc = h->bt_work.ensure(tag_plan_work_words(first) * sizeof(uint32_t))))
        return rc;
    {
        StageScope sc(h, IVFHNSW_STAGE_PLAN); // the plans and the gathers, accounted apart from the sweeps
        for (size_t q0 = 0, i = 0; q0 < nq; q0 += kExactChunk, i++) {
            StripPlan &sp = rs.plans[i];
            HIP_TRY(launch_tag_strip_plan(h->stream, d_tags + q0, std::min(kExactChunk, nq - q0), tr, h->bs_plan.as<unsigned char>() + i * plan_bytes,
                                          rs.bound, h->bt_work.as<uint32_t>(), &sp));
            sp.map_strip0 = (uint32_t)(i * rs.bound);
            // the queries as the store holds its rows, in strip order; a padding row repeats the chunk's first query
            HIP_TRY(launch_f16_store_rows(h->stream, d_queries + q0 * row_stride, row_stride, h->ex_q.as<unsigned char>() + i * rs.bound * 32 * d * 2,
                                          h->ex_qn.as<float>() + i * rs.bound * 32, rs.bound * 32, (int)d, sp.strip_rows));
        }
    }
    HIP_TRY(hipMemsetAsync(h->xr_slices.p, 0, len * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->xr_tot.p, 0, sizeof(unsigned long long), h->stream));
    if ((rc = exact_range_f16_strips_pass(h, b, rs, false, nq, radius, map_shift, nullptr, nullptr, 0)))
        return rc;
    unsigned long long tot = 0;
    if ((rc = exact_range_total(h, who, len, &tot)))
        return rc;
    RangeOut out;
    if ((rc = out.reserve(h, tot)))
        return rc;
    HIP_TRY(launch_range_lims(h->stream, h->xr_slices.as<uint32_t>(), (int)nq, nsplit, d_lims));
    if (tot && (rc = exact_range_f16_strips_pass(h, b, rs, true, nq, radius, map_shift, out.dist(h), out.lab(h), (size_t)tot)))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    out.commit(h, tot);
    *total = tot;
    return IVFHNSW_OK;
}

int exact_range_f16_tags_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, const uint16_t *query_tags, float radius,
                              uint64_t *lims, uint64_t *total, bool on_device)
{
    if (!query_tags)
        return exact_range_f16_impl(h, nq, queries, row_stride, radius, lims, total, on_device);
    const char *who = on_device ? "exact_range_search_f16_tags_dev" : "exact_range_search_f16_tags";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "exact_range_search_tags", &b);
    if (rc)
        return rc;
    if (std::isnan(radius))
        return fail(IVFHNSW_ERR_INVALID, "%s: the radius is NaN", who);
    TagRows tr;
    size_t in_use = 0;
    if ((rc = base_tags_call(b, who, &tr, &in_use)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, on_device ? nullptr : lims, on_device ? lims : nullptr, total);
    const size_t d = b->base_d;
    if (!queries || !lims || !total)
        return fail(IVFHNSW_ERR_INVALID, "%s: null queries, lims or total", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (nq > kMaxBatchAll)
        return fail(IVFHNSW_ERR_INVALID, "%s is limited to %zu queries per call", who, kMaxBatchAll);
    if (on_device && (((uintptr_t)queries & 3) || ((uintptr_t)lims & 7) || ((uintptr_t)query_tags & 1)))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries must be 4-byte, lims 8-byte and query tags 2-byte aligned", who);
    if (on_device)
        return exact_range_f16_tags_dev(h, b, who, nq, queries, row_stride, query_tags, tr, in_use, radius, lims, total);
    if ((rc = h->ex_raw.ensure(nq * d * sizeof(float))) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))) ||
        (rc = h->bs_qslots.ensure(nq * sizeof(uint16_t))))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), queries, row_stride * sizeof(float), d * sizeof(float), nq,
                             hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, query_tags, nq * sizeof(uint16_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = exact_range_f16_tags_dev(h, b, who, nq, h->ex_raw.as<float>(), d, h->bs_qslots.as<uint16_t>(), tr, in_use, radius,
                                       h->xr_lims.as<uint64_t>(), total)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// ---------------------------------------------------------------------------------------------------------------------
// ... with an interval of base values per query: the same sequence around the two kernels a value plan
// takes.  Per chunk of kExactChunk queries the value plan is made once and kept for both passes -- the plan, the windows of
// its strip rows and its place in the tile map -- with chunk i's gathered queries at row i * bound * 32 of h->ex_q /
// h->ex_qn.  The windowed strips write a query's results in (value, row) order: where any chunk has one and there are
// results, they are gathered by label behind the fill pass, as exact_range_dev of the uint8 store does (RangeByLabel).

// The splits of the windowed launch over `rows` padded strip rows and a store of nx rows, the longest span a strip can have.
// exact_splits_for(rows, nx, 1) -- the uint8 sweep's rule, a workgroup of four strips -- asks for enough workgroups for two
// per CU and rounds UP: 10 000 queries are 79 workgroups, 7 splits, 553 workgroups on 512 places, and the 41 left over run
// a second round alone.  This rule rounds DOWN, to the most splits whose workgroups all run at once (6 there: measured 23 %
// faster than 7 on long windows and level with it on short ones); a split never shorter than 4096 columns.
// Two workgroups per CU is what the registers give up to d = 160; beyond it the count has not been measured.
int exact_range_f16_window_splits_for(size_t rows, size_t nx)
{
    const size_t blocks = (rows + 127) / 128, max_s = std::min<size_t>(64, std::max<size_t>(1, (nx + 4095) / 4096));
    return (int)std::max<size_t>(1, std::min(max_s, 512 / blocks));
}

// device pointers, the arguments checked (nq > 0)
int exact_range_f16_values_dev(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const char *who, size_t nq, const float *d_queries, size_t row_stride,
                               const uint32_t *d_ranges, const ValueRows &vr, float radius, uint64_t *d_lims, uint64_t *total)
{
    const size_t d = b->base_d, n = b->base_n, first = std::min(nq, kExactChunk), nchunks = (nq + kExactChunk - 1) / kExactChunk;
    F16RangeStrips rs;
    rs.bound = sweep_value_strip_bound(first);
    // the windowed sweep only where a row holds a value
    rs.forms = 1u << kSweepColsDense | (vr.vals ? 1u << kSweepColsIndirect : 0u);
    // Dense: the plain call's rule over the chunk's queries padded to a strip; windowed: its own rule over the rows of
    // every strip the plan can have
    rs.ns_dense = exact_range_f16_splits_for((first + 31) / 32 * 32, n, d);
    rs.ns_ind = vr.vals ? exact_range_f16_window_splits_for(rs.bound * 32, n) : 1;
    if (h->opt_exact_splits > 0)
        rs.ns_dense = rs.ns_ind = h->opt_exact_splits;
    rs.plans.resize(nchunks);
    rs.wins.assign(nchunks, nullptr);
    std::vector<uint32_t> win_range(2 * nchunks, 0u); // per chunk the strips of its plan that are windowed, read back with the count
    const int nsplit = std::max(rs.ns_dense, rs.ns_ind); // the one width of the slices table
    const size_t len = nq * (size_t)nsplit + 1, rows = nchunks * rs.bound * 32, plan_bytes = sweep_value_plan_bytes(rs.bound);
    size_t map_bytes = 0;
    const int map_shift = exact_range_map_shift(rows, n, 2 * d, nsplit, &map_bytes);
    map_bytes = rows / 32 * exact_range_f16_strips_map_words(n, rs.ns_dense, rs.ns_ind, map_shift) * sizeof(uint32_t);
    int rc;
    if ((rc = h->ex_q.ensure(rows * d * 2)) || (rc = h->ex_qn.ensure(rows * sizeof(float))) ||
        (rc = h->xr_slices.ensure(len * sizeof(uint32_t))) || (rc = h->xr_part.ensure(append_scan_parts(len) * sizeof(uint32_t))) ||
        (rc = h->xr_tot.ensure(sizeof(unsigned long long))) || (h->opt_exact_range_map && (rc = h->xr_map.ensure(map_bytes))) ||
        (rc = h->bs_plan.ensure(nchunks * plan_bytes)) || (rc = h->bv_work.ensure(value_plan_work_words(first) * sizeof(uint32_t))))
        return rc;
    {
        StageScope sc(h, IVFHNSW_STAGE_PLAN); // the plans and the gathers, accounted apart from the sweeps
        for (size_t q0 = 0, i = 0; q0 < nq; q0 += kExactChunk, i++) {
            StripPlan &sp = rs.plans[i];
            HIP_TRY(launch_value_strip_plan(h->stream, d_ranges + 2 * q0, std::min(kExactChunk, nq - q0), vr,
                                            h->bs_plan.as<unsigned char>() + i * plan_bytes, rs.bound, h->bv_work.as<uint32_t>(), &sp,
                                            &rs.wins[i]));
            HIP_TRY(hipMemcpyAsync(&win_range[2 * i], sp.hdr->lay.range[kSweepColsIndirect], 2 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                                   h->stream));
            sp.map_strip0 = (uint32_t)(i * rs.bound);
            // the queries as the store holds its rows, in strip order; a padding row repeats the chunk's first query
            HIP_TRY(launch_f16_store_rows(h->stream, d_queries + q0 * row_stride, row_stride, h->ex_q.as<unsigned char>() + i * rs.bound * 32 * d * 2,
                                          h->ex_qn.as<float>() + i * rs.bound * 32, rs.bound * 32, (int)d, sp.strip_rows));
        }
    }
    HIP_TRY(hipMemsetAsync(h->xr_slices.p, 0, len * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->xr_tot.p, 0, sizeof(unsigned long long), h->stream));
    if ((rc = exact_range_f16_strips_pass(h, b, rs, false, nq, radius, map_shift, nullptr, nullptr, 0)))
        return rc;
    unsigned long long tot = 0;
    if ((rc = exact_range_total(h, who, len, &tot))) // (the synchronisation that brings win_range)
        return rc;
    bool windowed = false;
    for (size_t i = 0; i < nchunks; i++)
        windowed |= (rs.forms >> kSweepColsIndirect & 1u) && win_range[2 * i + 1] > win_range[2 * i];
    RangeOut out;
    RangeByLabel by_label;
    if ((rc = out.reserve(h, tot)) || (tot && windowed && (rc = by_label.reserve(tot))))
        return rc;
    HIP_TRY(launch_range_lims(h->stream, h->xr_slices.as<uint32_t>(), (int)nq, nsplit, d_lims));
    if (tot && (rc = exact_range_f16_strips_pass(h, b, rs, true, nq, radius, map_shift, out.dist(h), out.lab(h), (size_t)tot)))
        return rc;
    if ((rc = by_label.run(h, d_lims, nq, tot, out)))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    by_label.commit(h, out);
    out.commit(h, tot);
    *total = tot;
    return IVFHNSW_OK;
}

int exact_range_f16_values_impl(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, const uint32_t *query_ranges, float radius,
                                uint64_t *lims, uint64_t *total, bool on_device)
{
    if (!query_ranges)
        return exact_range_f16_impl(h, nq, queries, row_stride, radius, lims, total, on_device);
    const char *who = on_device ? "exact_range_search_f16_values_dev" : "exact_range_search_f16_values";
    const ivfhnsw_gpu *b;
    int rc = exact_f16_guard(h, who, "exact_range_search_values", &b);
    if (rc)
        return rc;
    if (std::isnan(radius))
        return fail(IVFHNSW_ERR_INVALID, "%s: the radius is NaN", who);
    ValueRows vr;
    if ((rc = base_values_call(b, who, &vr)))
        return rc;
    if (nq == 0)
        return exact_range_none(h, on_device ? nullptr : lims, on_device ? lims : nullptr, total);
    const size_t d = b->base_d;
    if (!queries || !lims || !total)
        return fail(IVFHNSW_ERR_INVALID, "%s: null queries, lims or total", who);
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);
    if (nq > kMaxBatchAll)
        return fail(IVFHNSW_ERR_INVALID, "%s is limited to %zu queries per call", who, kMaxBatchAll);
    if (on_device && (((uintptr_t)queries & 3) || ((uintptr_t)lims & 7) || ((uintptr_t)query_ranges & 7)))
        return fail(IVFHNSW_ERR_INVALID, "%s: queries must be 4-byte, lims 8-byte and query ranges 8-byte aligned", who);
    if (on_device)
        return exact_range_f16_values_dev(h, b, who, nq, queries, row_stride, query_ranges, vr, radius, lims, total);
    if ((rc = h->ex_raw.ensure(nq * d * sizeof(float))) || (rc = h->xr_lims.ensure((nq + 1) * sizeof(uint64_t))) ||
        (rc = h->bs_qslots.ensure(nq * 2 * sizeof(uint32_t))))
        return rc;
    HIP_TRY(hipMemcpy2DAsync(h->ex_raw.p, d * sizeof(float), queries, row_stride * sizeof(float), d * sizeof(float), nq,
                             hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->bs_qslots.p, query_ranges, nq * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if ((rc = exact_range_f16_values_dev(h, b, who, nq, h->ex_raw.as<float>(), d, h->bs_qslots.as<uint32_t>(), vr, radius,
                                         h->xr_lims.as<uint64_t>(), total)))
        return rc;
    HIP_TRY(hipMemcpyAsync(lims, h->xr_lims.p, (nq + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

} // namespace

int ivfhnsw_gpu_upload_base_f16(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const float *rows,
                                size_t row_stride)
{
    return upload_base_f16_impl(h, n, d, first, count, rows, row_stride, false);
}

int ivfhnsw_gpu_upload_base_f16_dev(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const float *d_rows,
                                    size_t row_stride)
{
    return upload_base_f16_impl(h, n, d, first, count, d_rows, row_stride, true);
}

int ivfhnsw_gpu_base_kind(const ivfhnsw_gpu *h)
{
    if (!h)
        return IVFHNSW_BASE_NONE;
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    return b->base_n ? b->base_kind : IVFHNSW_BASE_NONE;
}

int ivfhnsw_gpu_exact_search_f16(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k, float *distances,
                                 int64_t *labels)
{
    return exact_f16_impl(h, nq, queries, row_stride, k, distances, labels, false);
}

int ivfhnsw_gpu_exact_search_f16_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride, size_t k,
                                     float *d_distances, int64_t *d_labels)
{
    return exact_f16_impl(h, nq, d_queries, row_stride, k, d_distances, d_labels, true);
}

// ---- with a base tag per query; query_tags == NULL is the plain call

int ivfhnsw_gpu_exact_search_f16_tags(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k,
                                      const uint16_t *query_tags, float *distances, int64_t *labels)
{
    return exact_f16_tags_impl(h, nq, queries, row_stride, k, query_tags, distances, labels, false);
}

int ivfhnsw_gpu_exact_search_f16_tags_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride, size_t k,
                                          const uint16_t *d_query_tags, float *d_distances, int64_t *d_labels)
{
    return exact_f16_tags_impl(h, nq, d_queries, row_stride, k, d_query_tags, d_distances, d_labels, true);
}

// ---- with a base tag and an interval of base values per query; a NULL array leaves the other's call

int ivfhnsw_gpu_exact_search_f16_tags_values(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k,
                                             const uint16_t *query_tags, const uint32_t *query_ranges, float *distances, int64_t *labels)
{
    return exact_f16_tags_values_impl(h, nq, queries, row_stride, k, query_tags, query_ranges, distances, labels, false);
}

int ivfhnsw_gpu_exact_search_f16_tags_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride, size_t k,
                                                 const uint16_t *d_query_tags, const uint32_t *d_query_ranges, float *d_distances,
                                                 int64_t *d_labels)
{
    return exact_f16_tags_values_impl(h, nq, d_queries, row_stride, k, d_query_tags, d_query_ranges, d_distances, d_labels, true);
}

// ---- with an interval of base values per query; query_ranges == NULL is the plain call

int ivfhnsw_gpu_exact_search_f16_values(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, size_t k,
                                        const uint32_t *query_ranges, float *distances, int64_t *labels)
{
    return exact_f16_values_impl(h, nq, queries, row_stride, k, query_ranges, distances, labels, false);
}

int ivfhnsw_gpu_exact_search_f16_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride, size_t k,
                                            const uint32_t *d_query_ranges, float *d_distances, int64_t *d_labels)
{
    return exact_f16_values_impl(h, nq, d_queries, row_stride, k, d_query_ranges, d_distances, d_labels, true);
}

int ivfhnsw_gpu_exact_range_search_f16(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride, float radius,
                                       uint64_t *lims, uint64_t *total)
{
    return exact_range_f16_impl(h, nq, queries, row_stride, radius, lims, total, false);
}

int ivfhnsw_gpu_exact_range_search_f16_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride, float radius,
                                           uint64_t *d_lims, uint64_t *total)
{
    return exact_range_f16_impl(h, nq, d_queries, row_stride, radius, d_lims, total, true);
}

// ---- with a base tag per query; query_tags == NULL is the plain call

int ivfhnsw_gpu_exact_range_search_f16_tags(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride,
                                            const uint16_t *query_tags, float radius, uint64_t *lims, uint64_t *total)
{
    return exact_range_f16_tags_impl(h, nq, queries, row_stride, query_tags, radius, lims, total, false);
}

int ivfhnsw_gpu_exact_range_search_f16_tags_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride,
                                                const uint16_t *d_query_tags, float radius, uint64_t *d_lims, uint64_t *total)
{
    return exact_range_f16_tags_impl(h, nq, d_queries, row_stride, d_query_tags, radius, d_lims, total, true);
}

// ---- with an interval of base values per query; query_ranges == NULL is the plain call

int ivfhnsw_gpu_exact_range_search_f16_values(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t row_stride,
                                              const uint32_t *query_ranges, float radius, uint64_t *lims, uint64_t *total)
{
    return exact_range_f16_values_impl(h, nq, queries, row_stride, query_ranges, radius, lims, total, false);
}

int ivfhnsw_gpu_exact_range_search_f16_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t row_stride,
                                                  const uint32_t *d_query_ranges, float radius, uint64_t *d_lims, uint64_t *total)
{
    return exact_range_f16_values_impl(h, nq, d_queries, row_stride, d_query_ranges, radius, d_lims, total, true);
}
