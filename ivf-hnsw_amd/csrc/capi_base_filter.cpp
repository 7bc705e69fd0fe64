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
    ScopedBuf cnt, part;
    const size_t len = sweep_pass_words(n) + 1;
    int rc;
    if ((rc = rows.ensure(npass * sizeof(uint32_t))) == IVFHNSW_OK && (rc = cnt.ensure(len * sizeof(uint32_t))) == IVFHNSW_OK &&
        (rc = part.ensure(append_scan_parts(len) * sizeof(uint32_t))) == IVFHNSW_OK) {
        hipError_t e = launch_pass_rows(h->stream, words, n, cnt.as<uint32_t>(), part.as<uint32_t>(), rows.as<uint32_t>());
        if (e == hipSuccess)
            e = hipStreamSynchronize(h->stream); // the workspace goes with this scope
        if (e != hipSuccess)
            rc = fail(IVFHNSW_ERR_HIP, "base filter, pass rows: %s", hipGetErrorString(e));
    }
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

// what both forms of set_base_filter check first
static int set_base_filter_guard(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode, const char *who)
{
    int rc = filter_holder_guard(h, kBaseFilter, who, true);
    return rc ? rc : label_args_guard(n, labels, who, &mode);
}

// The set of d_labels [n] in device memory (n > 0: max_label = their maximum) under `mode` over the rows of h's store, built
// on the handle's stream beside whatever is installed: its pass words, the rows that pass, and their list where one is kept.
// What set_base_filter and set_base_filter_slot share; each installs the result in its own place.
static int build_pass_set(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode, ScopedBuf &words,
                          ScopedBuf &rows, unsigned long long *pass, bool *has_rows)
{
    const uint64_t rows_n = h->base_n;
    int rc;
    *pass = 0;
    {
        ScopedBuf bits; // gone before the rows are built
        if ((rc = labels_bitmap(h, n, d_labels, max_label, bits)) || (rc = words.ensure(sweep_pass_words(rows_n) * sizeof(uint32_t))) ||
            (rc = h->bf_count.ensure(sizeof(unsigned long long))))
            return rc;
        HIP_TRY(launch_pass_words(h->stream, bits.as<uint32_t>(), n ? label_bitmap_words(max_label) : 0, rows_n,
                                  mode == IVFHNSW_FILTER_DENY, words.as<uint32_t>(), h->bf_count.as<unsigned long long>()));
        // the one word that comes back: base_filter_info's count and the choice of form
        HIP_TRY(hipMemcpyAsync(pass, h->bf_count.p, sizeof(*pass), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    *has_rows = *pass > 0 && (sweep_pass_list_kept(*pass, rows_n) || h->opt_exact_filter_form == 1);
    if (*has_rows && (rc = build_pass_rows(h, words.as<uint32_t>(), rows_n, *pass, rows)))
        return rc;
    return IVFHNSW_OK;
}

// Words and rows are built beside the installed ones and swapped in when complete: any error leaves the earlier filter in
// force.
static int set_base_filter_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode)
{
    ScopedBuf words, rows;
    unsigned long long pass = 0;
    bool has_rows = false;
    if (int rc = build_pass_set(h, n, d_labels, max_label, mode, words, rows, &pass, &has_rows))
        return rc;
    words.install(h->bf_words); // the earlier filter's go with this scope
    rows.install(h->bf_rows);
    h->bf_mode = mode;
    h->bf_pass = pass;
    h->bf_has_rows = has_rows;
    h->bf_gen++;
    return IVFHNSW_OK;
}

// ---- base filter slots ------------------------------------------------------------------------------

void base_slots_drop(ivfhnsw_gpu *h)
{
    for (BaseSlot &s : h->bslots) {
        s.words.release();
        s.rows.release();
        s.mode = -1;
        s.pass = 0;
        s.has_rows = false;
    }
    h->bs_table.release();
}

// the entry of a slot: Indirect where the rule (or the option) asks for the list and the slot keeps one, else Masked;
// a slot that is not set or that no row passes sweeps nothing
static StripCols base_slot_entry(const ivfhnsw_gpu *h, const BaseSlot &s)
{
    if (s.mode < 0 || s.pass == 0)
        return {nullptr, 0, (uint32_t)kSweepColsNothing};
    if (s.has_rows && sweep_filter_form(s.pass, h->base_n, h->opt_exact_filter_form) == kSweepColsIndirect)
        return {s.rows.as<uint32_t>(), (uint32_t)s.pass, (uint32_t)kSweepColsIndirect};
    return {s.words.as<uint32_t>(), (uint32_t)h->base_n, (uint32_t)kSweepColsMasked};
}

int base_slots_table_write(ivfhnsw_gpu *h, bool create)
{
    if (!h->base_n || (!create && !h->bs_table.p))
        return IVFHNSW_OK;
    StripCols tab[kStripNone + 1];
    for (int i = 0; i < kStripSlots; i++)
        tab[i] = base_slot_entry(h, h->bslots[i]);
    tab[kStripNone] = {nullptr, (uint32_t)h->base_n, (uint32_t)kSweepColsDense};
    int rc = h->bs_table.ensure(sizeof(tab));
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream)); // exact calls in flight still read the table
    HIP_TRY(hipMemcpyAsync(h->bs_table.p, tab, sizeof(tab), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int base_slots_call(ivfhnsw_gpu *h, const ivfhnsw_gpu *b, const char *who, const StripCols **table, unsigned *forms)
{
    if (b->bf_mode >= 0)
        return fail(IVFHNSW_ERR_STATE, "%s: the store has a set_base_filter filter installed; a call is filtered by that or by "
                                       "slots, not both (clear_base_filter first)", who);
    if (!b->bs_table.p) {
        // no slot was set since the store came: the table of "none" alone, written on the holder by whoever asks first
        ivfhnsw_gpu *holder = h->parent ? h->parent : h;
        if (int rc = base_slots_table_write(holder, true))
            return rc;
    }
    *table = b->bs_table.as<StripCols>();
    *forms = 1u << kSweepColsDense;
    for (const BaseSlot &s : b->bslots)
        if (const StripCols e = base_slot_entry(b, s); e.form != kSweepColsNothing)
            *forms |= 1u << e.form;
    return IVFHNSW_OK;
}

static int base_slot_args(unsigned slot, const char *who)
{
    if (slot >= IVFHNSW_FILTER_SLOTS)
        return fail(IVFHNSW_ERR_INVALID, "%s: slot %u, a handle has slots 0..%d", who, slot, IVFHNSW_FILTER_SLOTS - 1);
    return IVFHNSW_OK;
}

// as set_base_filter_core, into slot `slot`; the table is reserved before anything is installed
static int set_base_slot_core(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode)
{
    ScopedBuf words, rows;
    unsigned long long pass = 0;
    bool has_rows = false;
    int rc;
    if ((rc = build_pass_set(h, n, d_labels, max_label, mode, words, rows, &pass, &has_rows)) ||
        (rc = h->bs_table.ensure(sizeof(StripCols) * (kStripNone + 1))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream)); // exact calls in flight still read the slot's earlier set
    BaseSlot &s = h->bslots[slot];
    words.install(s.words); // the earlier set's go with this scope
    rows.install(s.rows);
    s.mode = mode;
    s.pass = pass;
    s.has_rows = has_rows;
    return base_slots_table_write(h, true);
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_set_base_filter(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode)
{
    int rc = set_base_filter_guard(h, n, labels, mode, "set_base_filter");
    if (rc)
        return rc;
    ScopedBuf stage; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_from_host(h, n, labels, stage, &mx)))
        return rc;
    return set_base_filter_core(h, n, stage.as<uint32_t>(), mx, mode);
}

int ivfhnsw_gpu_set_base_filter_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int mode)
{
    int rc = set_base_filter_guard(h, n, d_labels, mode, "set_base_filter_dev");
    if (rc)
        return rc;
    if ((uintptr_t)d_labels & 3)
        return fail(IVFHNSW_ERR_INVALID, "set_base_filter_dev: labels must be 4-byte aligned");
    uint32_t mx = 0;
    // the count's buffer at the size the mark wants it (not grown a second time there); the maximum comes through its first word
    if ((n && (rc = h->bf_count.ensure(sizeof(unsigned long long)))) || (rc = labels_max_dev(h, h->bf_count, n, d_labels, &mx)))
        return rc;
    return set_base_filter_core(h, n, d_labels, mx, mode);
}

int ivfhnsw_gpu_clear_base_filter(ivfhnsw_gpu *h)
{
    int rc = filter_holder_guard(h, kBaseFilter, "clear_base_filter", false);
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
    return label_set_info(b->bf_mode, b->bf_pass, b->base_n, b->base_n, mode, rows_passing, rows_total);
}

// ---- base filter slots

int ivfhnsw_gpu_set_base_filter_slot(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *labels, int mode)
{
    int rc = set_base_filter_guard(h, n, labels, mode, "set_base_filter_slot");
    if (rc || (rc = base_slot_args(slot, "set_base_filter_slot")))
        return rc;
    ScopedBuf stage; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_from_host(h, n, labels, stage, &mx)))
        return rc;
    return set_base_slot_core(h, slot, n, stage.as<uint32_t>(), mx, mode);
}

int ivfhnsw_gpu_set_base_filter_slot_dev(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *d_labels, int mode)
{
    int rc = set_base_filter_guard(h, n, d_labels, mode, "set_base_filter_slot_dev");
    if (rc || (rc = base_slot_args(slot, "set_base_filter_slot_dev")))
        return rc;
    if ((uintptr_t)d_labels & 3)
        return fail(IVFHNSW_ERR_INVALID, "set_base_filter_slot_dev: labels must be 4-byte aligned");
    uint32_t mx = 0;
    if ((n && (rc = h->bf_count.ensure(sizeof(unsigned long long)))) || (rc = labels_max_dev(h, h->bf_count, n, d_labels, &mx)))
        return rc;
    return set_base_slot_core(h, slot, n, d_labels, mx, mode);
}

int ivfhnsw_gpu_clear_base_filter_slot(ivfhnsw_gpu *h, int slot)
{
    int rc = filter_holder_guard(h, kBaseFilter, "clear_base_filter_slot", false);
    if (rc)
        return rc;
    if (slot < -1 || slot >= IVFHNSW_FILTER_SLOTS)
        return fail(IVFHNSW_ERR_INVALID, "clear_base_filter_slot: slot %d, a handle has slots 0..%d (-1: every slot)", slot,
                    IVFHNSW_FILTER_SLOTS - 1);
    HIP_TRY(hipStreamSynchronize(h->stream)); // exact calls in flight still read the words
    for (int i = 0; i < IVFHNSW_FILTER_SLOTS; i++)
        if (slot < 0 || slot == i) {
            BaseSlot &s = h->bslots[i];
            s.words.release();
            s.rows.release();
            s.mode = -1;
            s.pass = 0;
            s.has_rows = false;
        }
    return base_slots_table_write(h, false);
}

int ivfhnsw_gpu_base_filter_slot_info(ivfhnsw_gpu *h, unsigned slot, int *mode, uint64_t *rows_passing, uint64_t *rows_total)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    if (int rc = base_slot_args(slot, "base_filter_slot_info"))
        return rc;
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    return label_set_info(b->bslots[slot].mode, b->bslots[slot].pass, 0, b->base_n, mode, rows_passing, rows_total);
}
