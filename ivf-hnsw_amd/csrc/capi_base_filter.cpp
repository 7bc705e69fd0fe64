// The base filter of a handle's store: while it is installed the exact calls (capi_exact.cpp) answer as
// they would on a store that held only the passing rows, labels being the original row numbers.  A label is a row number.
// The set becomes a bitmap over [0, max label] with removal's kernels, the bitmap one PASS bit per row of the store with
// the mode folded in (pass words), and, when few rows pass, the ascending list of their numbers (pass rows); the sweeps
// read one or the other through a column map (sweep_steps.h).  Independent of the index filter (capi_filter.cpp), whose
// labels are ids.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

void base_filter_drop(ivfhnsw_gpu *h)
{
    h->bf_mode = -1;
    h->bf_pass = 0;
    h->bf_has_rows = false;
    h->bf_gen++;
    h->bf_words.release();
    h->bf_rows.release();
    h->bf_count.release();
}

// the passing rows of words [n rows, npass of them passing > 0] into rows (allocated here), on h's stream; workspace freed
static int build_pass_rows(ivfhnsw_gpu *h, const uint32_t *words, uint64_t n, uint64_t npass, DevBuf &rows)
{
    DevBuf cnt, part;
    const size_t len = sweep_pass_words(n) + 1;
    int rc;
    if ((rc = rows.ensure(npass * sizeof(uint32_t))) == IVFHNSW_OK && (rc = cnt.ensure(len * sizeof(uint32_t))) == IVFHNSW_OK &&
        (rc = part.ensure(append_scan_parts(len) * sizeof(uint32_t))) == IVFHNSW_OK) {
        hipError_t e = launch_pass_rows(h->stream, words, n, cnt.as<uint32_t>(), part.as<uint32_t>(), rows.as<uint32_t>());
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream); // the workspace goes below
        if (e != hipSuccess)
            rc = fail(IVFHNSW_ERR_HIP, "base filter, pass rows: %s", hipGetErrorString(e));
    }
    cnt.release();
    part.release();
    return rc;
}

int base_filter_cols(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, SweepCols *cols, size_t *nx)
{
    *cols = SweepCols{};
    *nx = b->base_n;
    if (b->bf_mode < 0)
        return IVFHNSW_OK;
    *nx = b->bf_pass;
    if (b->bf_pass == 0)
        return IVFHNSW_OK;
    cols->form = sweep_filter_form(b->bf_pass, b->base_n, h->opt_exact_filter_form);
    if (cols->form == kSweepColsMasked) {
        *nx = b->base_n;
        cols->data = b->bf_words.as<uint32_t>();
        return IVFHNSW_OK;
    }
    if (b->bf_has_rows) {
        cols->data = b->bf_rows.as<uint32_t>();
        return IVFHNSW_OK;
    }
    // forced to the list of a filter that keeps none: this handle builds its own, once per filter
    if (h->bf_own_of != b || h->bf_own_gen != b->bf_gen || !h->bf_own.p) {
        h->bf_own_of = nullptr;
        if (int rc = build_pass_rows(h, b->bf_words.as<uint32_t>(), b->base_n, b->bf_pass, h->bf_own))
            return rc;
        h->bf_own_of = b;
        h->bf_own_gen = b->bf_gen;
    }
    cols->data = h->bf_own.as<uint32_t>();
    return IVFHNSW_OK;
}

static int base_filter_state(ivfhnsw_gpu *h, const char *who)
{
    if (h && h->is_view)
        return fail(IVFHNSW_ERR_STATE, "%s: a base filter goes to the handle that holds the store, not to a view of it", who);
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->base_n)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_base", who);
    return IVFHNSW_OK;
}

static int check_args(size_t n, const uint32_t *labels, int mode, const char *who)
{
    if (n && !labels)
        return fail(IVFHNSW_ERR_INVALID, "%s: null labels", who);
    if (mode != IVFHNSW_FILTER_ALLOW && mode != IVFHNSW_FILTER_DENY)
        return fail(IVFHNSW_ERR_INVALID, "%s: mode %d is neither IVFHNSW_FILTER_ALLOW nor IVFHNSW_FILTER_DENY", who, mode);
    return IVFHNSW_OK;
}

// d_labels [n] in device memory (n > 0: max_label = their maximum), read on the handle's stream.  Words and rows are built
// beside the installed ones and swapped in when complete: any error leaves the earlier filter in force.
static int set_base_filter_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode)
{
    DevBuf bits, words, rows;
    const uint64_t rows_n = h->base_n;
    unsigned long long pass = 0;
    bool has_rows = false;
    auto build = [&]() -> int {
        int rc;
        const size_t bit_words = n ? (size_t)max_label / 32 + 1 : 0;
        if (n) {
            if ((rc = bits.ensure(bit_words * sizeof(uint32_t))))
                return rc;
            HIP_TRY(launch_remove_bits(h->stream, d_labels, n, max_label, bits.as<uint32_t>()));
        }
        if ((rc = words.ensure(sweep_pass_words(rows_n) * sizeof(uint32_t))) || (rc = h->bf_count.ensure(sizeof(unsigned long long))))
            return rc;
        HIP_TRY(launch_pass_words(h->stream, n ? bits.as<uint32_t>() : nullptr, bit_words, rows_n, mode == IVFHNSW_FILTER_DENY,
                                  words.as<uint32_t>(), h->bf_count.as<unsigned long long>()));
        // the one word that comes back: base_filter_info's count and the choice of form
        HIP_TRY(hipMemcpyAsync(&pass, h->bf_count.p, sizeof(pass), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        bits.release();
        has_rows = pass > 0 && (sweep_pass_list_kept(pass, rows_n) || h->opt_exact_filter_form == 1);
        return has_rows ? build_pass_rows(h, words.as<uint32_t>(), rows_n, pass, rows) : IVFHNSW_OK;
    };
    if (int rc = build()) {
        bits.release();
        words.release();
        rows.release();
        return rc;
    }
    std::swap(h->bf_words, words);
    std::swap(h->bf_rows, rows);
    words.release(); // the earlier filter's
    rows.release();
    h->bf_mode = mode;
    h->bf_pass = pass;
    h->bf_has_rows = has_rows;
    h->bf_gen++;
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_set_base_filter(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode)
{
    int rc = base_filter_state(h, "set_base_filter");
    if (rc || (rc = check_args(n, labels, mode, "set_base_filter")))
        return rc;
    uint32_t mx = 0;
    for (size_t i = 0; i < n; i++)
        mx = std::max(mx, labels[i]);
    if (n) {
        if ((rc = h->bf_labels.ensure(n * sizeof(uint32_t))))
            return rc;
        HIP_TRY(hipMemcpyAsync(h->bf_labels.p, labels, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    }
    rc = set_base_filter_core(h, n, h->bf_labels.as<uint32_t>(), mx, mode);
    h->bf_labels.release(); // staging of this call only
    return rc;
}

int ivfhnsw_gpu_set_base_filter_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int mode)
{
    int rc = base_filter_state(h, "set_base_filter_dev");
    if (rc || (rc = check_args(n, d_labels, mode, "set_base_filter_dev")))
        return rc;
    if ((uintptr_t)d_labels & 3)
        return fail(IVFHNSW_ERR_INVALID, "set_base_filter_dev: labels must be 4-byte aligned");
    uint32_t mx = 0;
    if (n) {
        if ((rc = h->bf_count.ensure(sizeof(unsigned long long))))
            return rc;
        HIP_TRY(hipMemsetAsync(h->bf_count.p, 0, sizeof(uint32_t), h->stream));
        HIP_TRY(launch_remove_max(h->stream, d_labels, n, h->bf_count.as<uint32_t>()));
        HIP_TRY(hipMemcpyAsync(&mx, h->bf_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return set_base_filter_core(h, n, d_labels, mx, mode);
}

int ivfhnsw_gpu_clear_base_filter(ivfhnsw_gpu *h)
{
    if (h && h->is_view)
        return fail(IVFHNSW_ERR_STATE, "clear_base_filter: a base filter goes to the handle that holds the store, not to a view of it");
    int rc = bind(h);
    if (rc)
        return rc;
    if (h->bf_mode < 0)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // exact calls in flight still read the words
    base_filter_drop(h);
    h->bf_own.release();
    h->bf_own_of = nullptr;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_base_filter_info(ivfhnsw_gpu *h, int *mode, uint64_t *rows_passing, uint64_t *rows_total)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    if (mode)
        *mode = b->bf_mode;
    if (rows_passing)
        *rows_passing = b->bf_mode >= 0 ? b->bf_pass : b->base_n;
    if (rows_total)
        *rows_total = b->base_n;
    return IVFHNSW_OK;
}
