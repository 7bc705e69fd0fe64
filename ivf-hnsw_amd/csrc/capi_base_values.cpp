// Base values: one uint32 per row of a handle's store, the ground truth of the index's row values (3.24).
// An exact _values call (capi_exact.cpp) answers every query as the plain call would with set_base_filter({rows whose
// value lies in the query's interval}, ALLOW) installed.  The holder keeps the value of every row and ALL row numbers
// ordered by (value, row), a valueless row last at 0xffffffff: an interval is then one window of positions of that order
// (sweep_plan_math.h sweep_value_window), which the windowed column map sweeps (sweep_steps.h).  Both arrays are rebuilt by
// every set call -- a stable sort of the row numbers by value.  Independent of the base filter, of its slots, of the base
// tags and of the index's row values (capi_filter.cpp), whose labels are ids.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

void base_values_drop(ivfhnsw_gpu *h)
{
    h->bv_valued = 0;
    h->bv_vals.release();
    h->bv_rows.release();
}

int base_values_call(const ivfhnsw_gpu *b, const char *who, ValueRows *vr)
{
    if (b->bf_mode >= 0)
        return fail(IVFHNSW_ERR_STATE, "%s: the store has a set_base_filter filter installed; a call is filtered by that or by "
                                       "values, not both (clear_base_filter first)", who);
    *vr = ValueRows{};
    vr->n = (uint32_t)b->base_n;
    if (b->bv_vals.p) {
        vr->vals = b->bv_vals.as<uint32_t>();
        vr->rows = b->bv_rows.as<uint32_t>();
    }
    return IVFHNSW_OK;
}

static int base_values_args(size_t n, const uint32_t *rows, const uint32_t *values, const char *who)
{
    if (n && (!rows || !values))
        return fail(IVFHNSW_ERR_INVALID, "%s: null rows or values", who);
    return IVFHNSW_OK;
}

// the window of (lo, hi) in holder b's row order, found on the device by the function the plan uses
static int base_values_window(ivfhnsw_gpu *h, const ValueRows &vr, uint32_t lo, uint32_t hi, StripWin *w)
{
    ScopedBuf work; // of this call only: the interval, then its window
    int rc = work.ensure(4 * sizeof(uint32_t));
    if (rc)
        return rc;
    const uint32_t pair[2] = {lo, hi};
    HIP_TRY(hipMemcpyAsync(work.p, pair, sizeof(pair), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_value_windows(h->stream, work.as<uint32_t>(), 1, vr, reinterpret_cast<StripWin *>(work.as<uint32_t>() + 2)));
    HIP_TRY(hipMemcpyAsync(w, work.as<uint32_t>() + 2, sizeof(*w), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// d_rows / d_values [n] in device memory.  The new value array (the installed one's entries, or valueless, then the n values
// scattered in) and the row order are built beside the installed ones -- 12 bytes per row: the values and the sort's two
// permutations, one of which is installed -- and swapped in when nothing can fail any more.  A row given two different
// values keeps one of them, which the check behind the scatter finds.
static int set_base_values_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_rows, const uint32_t *d_values)
{
    if (n == 0)
        return IVFHNSW_OK;
    const uint64_t N = h->base_n;
    ScopedBuf vals, ids_a, ids_b, work; // work: of this call only (the conflict word, the sort's histograms)
    int rc;
    const size_t hist_words = 256 * ((N + kKmeansTile - 1) / kKmeansTile);
    if ((rc = vals.ensure(N * sizeof(uint32_t))) || (rc = ids_a.ensure(N * sizeof(uint32_t))) || (rc = ids_b.ensure(N * sizeof(uint32_t))) ||
        (rc = work.ensure((4 + hist_words) * sizeof(uint32_t))))
        return rc;
    if (h->bv_vals.p)
        HIP_TRY(hipMemcpyAsync(vals.p, h->bv_vals.p, N * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    else // 0xffffffff: IVFHNSW_VALUE_NONE
        HIP_TRY(hipMemsetAsync(vals.p, 0xff, N * sizeof(uint32_t), h->stream));
    uint32_t *word = work.as<uint32_t>(), *hist = word + 4;
    uint32_t conflict = 0;
    HIP_TRY(launch_base_values_apply(h->stream, d_rows, d_values, n, N, vals.as<uint32_t>(), word));
    HIP_TRY(hipMemcpyAsync(&conflict, word, sizeof(conflict), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (conflict)
        return fail(IVFHNSW_ERR_INVALID, "set_base_values: a row is given two different values in one call");
    uint32_t *sorted = nullptr;
    HIP_TRY(launch_base_values_index(h->stream, vals.as<uint32_t>(), N, ids_a.as<uint32_t>(), ids_b.as<uint32_t>(), hist, &sorted));
    // the rows that hold a value: the start of the window of 0xffffffff alone
    ValueRows vr;
    vr.vals = vals.as<uint32_t>();
    vr.rows = sorted;
    vr.n = (uint32_t)N;
    StripWin none;
    if ((rc = base_values_window(h, vr, IVFHNSW_VALUE_NONE, IVFHNSW_VALUE_NONE, &none)))
        return rc; // (drains the stream: the order is complete; exact calls in flight still read the earlier arrays)
    vals.install(h->bv_vals); // the earlier arrays go with this scope
    (sorted == ids_a.as<uint32_t>() ? ids_a : ids_b).install(h->bv_rows);
    h->bv_valued = none.a;
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_set_base_values(ivfhnsw_gpu *h, size_t n, const uint32_t *rows, const uint32_t *values)
{
    int rc = filter_holder_guard(h, kBaseFilter, "set_base_values", true);
    if (rc || (rc = base_values_args(n, rows, values, "set_base_values")))
        return rc;
    ScopedBuf stage_r, stage_v; // of this call only
    if (n && ((rc = stage_in(h, stage_r, rows, n * sizeof(uint32_t))) || (rc = stage_in(h, stage_v, values, n * sizeof(uint32_t)))))
        return rc;
    return set_base_values_core(h, n, stage_r.as<uint32_t>(), stage_v.as<uint32_t>());
}

int ivfhnsw_gpu_set_base_values_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_rows, const uint32_t *d_values)
{
    int rc = filter_holder_guard(h, kBaseFilter, "set_base_values_dev", true);
    if (rc || (rc = base_values_args(n, d_rows, d_values, "set_base_values_dev")))
        return rc;
    if (((uintptr_t)d_rows & 3) || ((uintptr_t)d_values & 3))
        return fail(IVFHNSW_ERR_INVALID, "set_base_values_dev: rows and values must be 4-byte aligned");
    return set_base_values_core(h, n, d_rows, d_values);
}

int ivfhnsw_gpu_clear_base_values(ivfhnsw_gpu *h)
{
    int rc = filter_holder_guard(h, kBaseFilter, "clear_base_values", false);
    if (rc)
        return rc;
    if (!h->bv_vals.p)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // exact calls in flight still read the arrays
    base_values_drop(h);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_base_values_info(ivfhnsw_gpu *h, uint64_t *rows_valued, uint64_t *rows_total)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    if (rows_valued)
        *rows_valued = b->bv_valued;
    if (rows_total)
        *rows_total = b->base_n;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_base_value_rows(ivfhnsw_gpu *h, uint32_t lo, uint32_t hi, uint64_t *rows)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!rows)
        return fail(IVFHNSW_ERR_INVALID, "base_value_rows: a null result");
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    if (!b->base_n)
        return fail(IVFHNSW_ERR_STATE, "base_value_rows before upload_base");
    ValueRows vr;
    vr.n = (uint32_t)b->base_n;
    if (b->bv_vals.p) {
        vr.vals = b->bv_vals.as<uint32_t>();
        vr.rows = b->bv_rows.as<uint32_t>();
    }
    StripWin w;
    if ((rc = base_values_window(h, vr, lo, hi, &w)))
        return rc;
    *rows = w.b - w.a;
    return IVFHNSW_OK;
}
