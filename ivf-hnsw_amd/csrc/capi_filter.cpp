// The label filter of a handle: searches return only rows whose id is in an allowed set, or is not in a
// denied one.  The set becomes a bitmap over [0, max label], the bitmap one PASS bit per resident row, and the filtered
// forms of the scan kernels read that bit beside the row's norm code.  The bitmap stays with the handle so that in-place
// updates can judge the rows of their new arrays (ListArrays::mark_filter, capi_internal.h).  Filter slots (3.19) and
// row tags (3.21) and row values (3.24), the three per-query forms, and the call that reads tags AND values (3.26)
// live here too.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

static size_t mask_bytes(uint64_t n_local) { return (size_t)std::max<uint64_t>((n_local + 63) / 64, 1) * sizeof(uint64_t); }

// mark with an explicit label set (bits null = the empty set) rather than the handle's: set_filter builds beside the old one
static int mark_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, const uint32_t *bits, uint32_t max_label,
                     int mode, DevBuf &mask, uint64_t *pass)
{
    int rc;
    if ((rc = mask.ensure(mask_bytes(n_local))) || (rc = h->f_count.ensure(sizeof(unsigned long long))))
        return rc;
    unsigned long long cnt = 0;
    HIP_TRY(launch_filter_mark(h->stream, ids, n_local, bits, max_label, mode == IVFHNSW_FILTER_DENY,
                               mask.as<unsigned long long>(), h->f_count.as<unsigned long long>()));
    HIP_TRY(hipMemcpyAsync(&cnt, h->f_count.p, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *pass = cnt;
    return IVFHNSW_OK;
}

int filter_mark_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &mask, uint64_t *pass)
{
    return mark_rows(h, ids, n_local, h->filter.bitmap(), h->filter.max_label, h->filter.mode, mask, pass);
}

void filter_drop(ivfhnsw_gpu *h)
{
    h->filter.drop();
    h->fmask = nullptr;
    h->f_mask.release();
}

// the opening of the calls that set or clear a filter, a slot or the tags (what: "label filter" unless said)
static int filter_state(ivfhnsw_gpu *h, const char *who, bool need_upload = true, const char *what = "label filter")
{
    int rc = filter_holder_guard(h, kIndexFilter, who, need_upload);
    if (rc)
        return rc;
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle is shard %u of %u; sharded handles have no %s", who,
                    h->t.shard_rank, h->t.shard_world, what);
    return IVFHNSW_OK;
}

// d_labels [n] in device memory (n > 0: max_label = their maximum), read on the handle's stream.  The new bitmap and mask
// are built beside the installed ones and swapped in when complete: any error leaves the earlier filter in force.
static int set_filter_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode)
{
    ScopedBuf bits, mask;
    int rc;
    uint64_t pass = 0;
    if ((rc = labels_bitmap(h, n, d_labels, max_label, bits)) ||
        (rc = mark_rows(h, h->t.ids, h->n_local, bits.as<uint32_t>(), max_label, mode, mask, &pass)))
        return rc;
    h->filter.install(bits, n, max_label, mode, pass); // the earlier filter's bitmap and mask go with this scope
    mask.install(h->f_mask);
    h->fmask = h->f_mask.as<uint32_t>();
    return IVFHNSW_OK;
}

// ---- filter slots: the same label sets, up to IVFHNSW_FILTER_SLOTS of them, each marked into its own
// plane of fs_planes; a _slots call names a slot per query.

void slots_drop(ivfhnsw_gpu *h)
{
    h->fs = SlotMask{nullptr, 0, 0, nullptr};
    h->fs_planes.release();
    for (LabelSet &s : h->slots)
        s.drop();
}

int slots_mark_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &planes, uint64_t *pass)
{
    const uint32_t np = h->fs.nplanes;
    const uint64_t stride = slot_plane_stride(n_local);
    int rc;
    if ((rc = planes.ensure((size_t)np * stride * sizeof(uint32_t))) ||
        (rc = h->fs_count.ensure(kFilterSlots * sizeof(unsigned long long))))
        return rc;
    FilterSlotSets sets{};
    for (uint32_t s = 0; s < np; s++) {
        sets.bits[s] = h->slots[s].bitmap();
        sets.max_label[s] = h->slots[s].max_label;
        sets.set[s] = h->slots[s].mode >= 0;
        sets.deny[s] = h->slots[s].mode == IVFHNSW_FILTER_DENY;
    }
    if (n_local == 0) // no kernel runs: the one word of every plane
        HIP_TRY(hipMemsetAsync(planes.p, 0, (size_t)np * stride * sizeof(uint32_t), h->stream));
    unsigned long long cnt[kFilterSlots] = {0};
    HIP_TRY(launch_filter_mark_slots(h->stream, ids, n_local, sets, np, planes.as<unsigned long long>(), stride / 2,
                                     h->fs_count.as<unsigned long long>()));
    HIP_TRY(hipMemcpyAsync(cnt, h->fs_count.p, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    for (int s = 0; s < IVFHNSW_FILTER_SLOTS; s++)
        pass[s] = cnt[s];
    return IVFHNSW_OK;
}

int slots_call_guard(const ivfhnsw_gpu *h, const char *who, bool tags) { return slots_call_guard(h, who, tags ? 1 : 0); }

int slots_call_guard(const ivfhnsw_gpu *h, const char *who, int kind)
{
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle is shard %u of %u; sharded handles have no %s", who,
                    h->t.shard_rank, h->t.shard_world,
                    kind == 3 ? "row tags and values" : kind == 2 ? "row values" : kind == 1 ? "row tags" : "filter slots");
    if (h->filter.mode >= 0)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle has a set_filter filter installed; a call is filtered by that or by "
                                       "%s, not both (clear_filter first)", who,
                    kind == 3 ? "tags and values" : kind == 2 ? "values" : kind == 1 ? "tags" : "slots");
    return IVFHNSW_OK;
}

int pick_stage_in(ivfhnsw_gpu *h, const QueryPick &pick, size_t nq)
{
    int rc = h->fs_qslots.ensure(pick.bytes(nq));
    if (rc)
        return rc;
    return pick.each_array(nq, [&](const void *src, size_t at, size_t bytes) -> int {
        HIP_TRY(hipMemcpyAsync(h->fs_qslots.as<char>() + at, src, bytes, hipMemcpyHostToDevice, h->stream));
        return IVFHNSW_OK;
    });
}

int slots_bytes_guard(size_t nq, const uint8_t *query_slots, const char *who)
{
    for (size_t q = 0; q < nq; q++)
        if (query_slots[q] >= IVFHNSW_FILTER_SLOTS && query_slots[q] != IVFHNSW_SLOT_NONE)
            return fail(IVFHNSW_ERR_INVALID, "%s: query %zu names slot %u; slots are 0..%d or IVFHNSW_SLOT_NONE", who, q,
                        (unsigned)query_slots[q], IVFHNSW_FILTER_SLOTS - 1);
    return IVFHNSW_OK;
}

// the planes of the handle in a buffer of np planes (np above or below what it holds now), planes the handle lacks zero
static int planes_resized(ivfhnsw_gpu *h, uint32_t np, DevBuf &out)
{
    const size_t pb = (size_t)slot_plane_stride(h->n_local) * sizeof(uint32_t);
    const uint32_t keep = std::min(np, h->fs.nplanes);
    int rc = out.ensure((size_t)np * pb);
    if (rc)
        return rc;
    if (keep)
        HIP_TRY(hipMemcpyAsync(out.p, h->fs_planes.p, keep * pb, hipMemcpyDeviceToDevice, h->stream));
    if (np > keep)
        HIP_TRY(hipMemsetAsync(out.as<char>() + keep * pb, 0, (np - keep) * pb, h->stream));
    return IVFHNSW_OK;
}

// ... installed; the earlier planes go with the scope of `planes`
static void planes_install(ivfhnsw_gpu *h, ScopedBuf &planes, uint32_t np)
{
    planes.install(h->fs_planes);
    h->fs = SlotMask{np ? h->fs_planes.as<uint32_t>() : nullptr, np ? (uint32_t)slot_plane_stride(h->n_local) : 0u, np, nullptr};
}

// As set_filter_core, for one slot.  Label bitmap, the slot's mask and (a slot beyond the planes held) a larger set of
// planes are all built beside the installed state, which is touched only when nothing can fail any more: every error
// leaves every slot as it was.
static int set_slot_core(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode)
{
    ScopedBuf bits, mask, planes;
    int rc;
    uint64_t pass = 0;
    const bool grow = slot >= h->fs.nplanes;
    const size_t pb = (size_t)slot_plane_stride(h->n_local) * sizeof(uint32_t);
    if ((rc = labels_bitmap(h, n, d_labels, max_label, bits)) ||
        (rc = mark_rows(h, h->t.ids, h->n_local, bits.as<uint32_t>(), max_label, mode, mask, &pass)) ||
        (grow && (rc = planes_resized(h, slot + 1, planes))))
        return rc;
    // the last fallible step writes the plane: into the new buffer, or over the slot's own plane, which only this
    // slot's queries read
    char *dst = (grow ? planes.as<char>() : h->fs_planes.as<char>()) + (size_t)slot * pb;
    HIP_TRY(hipMemcpyAsync(dst, mask.p, pb, hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (grow)
        planes_install(h, planes, slot + 1);
    h->slots[slot].install(bits, n, max_label, mode, pass); // the slot's earlier set goes with this scope
    return IVFHNSW_OK;
}

// ---- row tags: disjoint sets as one uint16 per label value (tg_table, tg_labels entries), gathered into
// one uint16 per resident row (tg_rows), which the _tags scans compare with the query's tag.

void tags_drop(ivfhnsw_gpu *h)
{
    h->tg_labels = 0;
    h->row_tags = nullptr;
    h->tg_table.release();
    h->tg_rows.release();
}

// the tags of ids [n_local] from a table of table_n labels into out (grown here; never empty).  Returns with the stream drained.
static int gather_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, const uint16_t *table, uint64_t table_n, DevBuf &out)
{
    int rc = out.ensure((size_t)std::max<uint64_t>(n_local, 1) * sizeof(uint16_t));
    if (rc)
        return rc;
    HIP_TRY(launch_tags_gather(h->stream, ids, n_local, table, table_n, out.as<uint16_t>()));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int tags_gather_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &row_tags)
{
    return gather_rows(h, ids, n_local, h->tg_table.as<uint16_t>(), h->tg_labels, row_tags);
}

// d_labels / d_tags [n] in device memory, max_label their largest label.  As set_filter_core: the new table (the old one's
// entries, untagged beyond them, then the n tags scattered in) and the new row tags are built beside the installed ones
// and swapped in when nothing can fail any more.  A label given two different tags keeps one of them, which the check
// behind the scatter finds.
static int set_tags_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, const uint16_t *d_tags, uint32_t max_label)
{
    if (n == 0)
        return IVFHNSW_OK;
    const uint64_t held = h->tg_labels, span = std::max<uint64_t>(held, (uint64_t)max_label + 1);
    ScopedBuf table, rows, word; // word: of this call only
    int rc;
    if ((rc = table.ensure((size_t)span * sizeof(uint16_t))) || (rc = word.ensure(sizeof(uint32_t))))
        return rc;
    if (held)
        HIP_TRY(hipMemcpyAsync(table.p, h->tg_table.p, (size_t)held * sizeof(uint16_t), hipMemcpyDeviceToDevice, h->stream));
    if (span > held) // 0xffff: IVFHNSW_TAG_NONE
        HIP_TRY(hipMemsetAsync(table.as<uint16_t>() + held, 0xff, (size_t)(span - held) * sizeof(uint16_t), h->stream));
    uint32_t conflict = 0;
    HIP_TRY(launch_tags_scatter(h->stream, d_labels, d_tags, n, table.as<uint16_t>(), word.as<uint32_t>()));
    HIP_TRY(hipMemcpyAsync(&conflict, word.p, sizeof(conflict), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (conflict)
        return fail(IVFHNSW_ERR_INVALID, "set_tags: a label is given two different tags in one call");
    if ((rc = gather_rows(h, h->t.ids, h->n_local, table.as<uint16_t>(), span, rows)))
        return rc;
    table.install(h->tg_table); // the earlier table and row tags go with this scope
    rows.install(h->tg_rows);
    h->tg_labels = span;
    h->row_tags = h->tg_rows.as<uint16_t>();
    return IVFHNSW_OK;
}

static int tags_args(size_t n, const uint32_t *labels, const uint16_t *tags, const char *who)
{
    int rc = label_args_guard(n, labels, who);
    if (rc)
        return rc;
    if (n && !tags)
        return fail(IVFHNSW_ERR_INVALID, "%s: null tags", who);
    return IVFHNSW_OK;
}

// one counting pass over the row tags h reads: rows whose tag equals `tag`, or differs from it
static int tags_count(ivfhnsw_gpu *h, uint32_t tag, bool equal, uint64_t *out)
{
    if (!h->row_tags) { // no table: every row is untagged
        *out = (tag == IVFHNSW_TAG_NONE) == equal ? h->n_local : 0;
        return IVFHNSW_OK;
    }
    ScopedBuf word;
    int rc = word.ensure(sizeof(unsigned long long));
    if (rc)
        return rc;
    unsigned long long cnt = 0;
    HIP_TRY(launch_tags_count(h->stream, h->row_tags, h->n_local, tag, equal, word.as<unsigned long long>()));
    HIP_TRY(hipMemcpyAsync(&cnt, word.p, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out = cnt;
    return IVFHNSW_OK;
}

// ---- row values: a uint32 per label value (vl_table, vl_labels entries), gathered into one uint32 per
// resident row (vl_rows), which the _values scans judge against the query's interval.  Built as the tags are.

void values_drop(ivfhnsw_gpu *h)
{
    h->vl_labels = 0;
    h->row_values = nullptr;
    h->vl_table.release();
    h->vl_rows.release();
}

// the values of ids [n_local] from a table of table_n labels into out (grown here; never empty).  Returns with the stream drained.
static int gather_value_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, const uint32_t *table, uint64_t table_n,
                             DevBuf &out)
{
    int rc = out.ensure((size_t)std::max<uint64_t>(n_local, 1) * sizeof(uint32_t));
    if (rc)
        return rc;
    HIP_TRY(launch_values_gather(h->stream, ids, n_local, table, table_n, out.as<uint32_t>()));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int values_gather_rows(ivfhnsw_gpu *h, const uint32_t *ids, uint64_t n_local, DevBuf &row_values)
{
    return gather_value_rows(h, ids, n_local, h->vl_table.as<uint32_t>(), h->vl_labels, row_values);
}

// d_labels / d_values [n] in device memory, max_label their largest label.  As set_tags_core: the new table (the old
// one's entries, IVFHNSW_VALUE_NONE beyond them, then the n values scattered in) and the new row values are built beside
// the installed ones and swapped in when nothing can fail any more.
static int set_values_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, const uint32_t *d_values, uint32_t max_label)
{
    if (n == 0)
        return IVFHNSW_OK;
    const uint64_t held = h->vl_labels, span = std::max<uint64_t>(held, (uint64_t)max_label + 1);
    ScopedBuf table, rows, word; // word: of this call only
    int rc;
    if ((rc = table.ensure((size_t)span * sizeof(uint32_t))) || (rc = word.ensure(sizeof(uint32_t))))
        return rc;
    if (held)
        HIP_TRY(hipMemcpyAsync(table.p, h->vl_table.p, (size_t)held * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    if (span > held) // 0xffffffff: IVFHNSW_VALUE_NONE
        HIP_TRY(hipMemsetAsync(table.as<uint32_t>() + held, 0xff, (size_t)(span - held) * sizeof(uint32_t), h->stream));
    uint32_t conflict = 0;
    HIP_TRY(launch_values_scatter(h->stream, d_labels, d_values, n, table.as<uint32_t>(), word.as<uint32_t>()));
    HIP_TRY(hipMemcpyAsync(&conflict, word.p, sizeof(conflict), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (conflict)
        return fail(IVFHNSW_ERR_INVALID, "set_values: a label is given two different values in one call");
    if ((rc = gather_value_rows(h, h->t.ids, h->n_local, table.as<uint32_t>(), span, rows)))
        return rc;
    table.install(h->vl_table); // the earlier table and row values go with this scope
    rows.install(h->vl_rows);
    h->vl_labels = span;
    h->row_values = h->vl_rows.as<uint32_t>();
    return IVFHNSW_OK;
}

static int values_args(size_t n, const uint32_t *labels, const uint32_t *values, const char *who)
{
    int rc = label_args_guard(n, labels, who);
    if (rc)
        return rc;
    if (n && !values)
        return fail(IVFHNSW_ERR_INVALID, "%s: null values", who);
    return IVFHNSW_OK;
}

// one counting pass over the row values h reads: rows whose value lies in [lo, hi]
static int values_count(ivfhnsw_gpu *h, uint32_t lo, uint32_t hi, uint64_t *out)
{
    if (!h->row_values) { // no table: every row holds IVFHNSW_VALUE_NONE
        *out = lo <= hi && hi == IVFHNSW_VALUE_NONE ? h->n_local : 0;
        return IVFHNSW_OK;
    }
    ScopedBuf word;
    int rc = word.ensure(sizeof(unsigned long long));
    if (rc)
        return rc;
    unsigned long long cnt = 0;
    HIP_TRY(launch_values_count(h->stream, h->row_values, h->n_local, lo, hi, word.as<unsigned long long>()));
    HIP_TRY(hipMemcpyAsync(&cnt, word.p, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out = cnt;
    return IVFHNSW_OK;
}

// ... and over both: rows the conjunction of DESIGN.md 3.26 passes.  A missing table reads as NONE for every row.
static int tag_values_count(ivfhnsw_gpu *h, uint32_t tag, uint32_t lo, uint32_t hi, uint64_t *out)
{
    ScopedBuf word;
    int rc = word.ensure(sizeof(unsigned long long));
    if (rc)
        return rc;
    unsigned long long cnt = 0;
    HIP_TRY(launch_tag_values_count(h->stream, h->row_tags, h->row_values, h->n_local, tag, lo, hi, word.as<unsigned long long>()));
    HIP_TRY(hipMemcpyAsync(&cnt, word.p, sizeof(cnt), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *out = cnt;
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_set_filter(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode)
{
    int rc = filter_state(h, "set_filter");
    if (rc || (rc = label_args_guard(n, labels, "set_filter", &mode)))
        return rc;
    ScopedBuf stage; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_from_host(h, n, labels, stage, &mx)))
        return rc;
    return set_filter_core(h, n, stage.as<uint32_t>(), mx, mode);
}

int ivfhnsw_gpu_set_filter_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int mode)
{
    int rc = filter_state(h, "set_filter_dev");
    if (rc || (rc = label_args_guard(n, d_labels, "set_filter_dev", &mode)))
        return rc;
    if ((uintptr_t)d_labels & 3)
        return fail(IVFHNSW_ERR_INVALID, "set_filter_dev: labels must be 4-byte aligned");
    uint32_t mx = 0;
    // the count's buffer at the size the mark wants it (not grown a second time there); the maximum comes through its first word
    if ((n && (rc = h->f_count.ensure(sizeof(unsigned long long)))) || (rc = labels_max_dev(h, h->f_count, n, d_labels, &mx)))
        return rc;
    return set_filter_core(h, n, d_labels, mx, mode);
}

int ivfhnsw_gpu_clear_filter(ivfhnsw_gpu *h)
{
    int rc = filter_holder_guard(h, kIndexFilter, "clear_filter", false);
    if (rc)
        return rc;
    if (h->filter.mode < 0)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // searches in flight still read the mask (a split batch joins this stream)
    filter_drop(h);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_filter_info(ivfhnsw_gpu *h, int *mode, uint64_t *rows_passing, uint64_t *rows_total)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    return label_set_info(h->filter.mode, h->filter.pass, h->n_local, h->n_local, mode, rows_passing, rows_total);
}

// ---- filter slots

static int slot_args(unsigned slot, size_t n, const uint32_t *labels, int mode, const char *who)
{
    if (slot >= IVFHNSW_FILTER_SLOTS)
        return fail(IVFHNSW_ERR_INVALID, "%s: slot %u, a handle has slots 0..%d", who, slot, IVFHNSW_FILTER_SLOTS - 1);
    return label_args_guard(n, labels, who, &mode);
}

int ivfhnsw_gpu_set_filter_slot(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *labels, int mode)
{
    int rc = filter_state(h, "set_filter_slot");
    if (rc || (rc = slot_args(slot, n, labels, mode, "set_filter_slot")))
        return rc;
    ScopedBuf stage; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_from_host(h, n, labels, stage, &mx)))
        return rc;
    return set_slot_core(h, slot, n, stage.as<uint32_t>(), mx, mode);
}

int ivfhnsw_gpu_set_filter_slot_dev(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *d_labels, int mode)
{
    int rc = filter_state(h, "set_filter_slot_dev");
    if (rc || (rc = slot_args(slot, n, d_labels, mode, "set_filter_slot_dev")))
        return rc;
    if ((uintptr_t)d_labels & 3)
        return fail(IVFHNSW_ERR_INVALID, "set_filter_slot_dev: labels must be 4-byte aligned");
    uint32_t mx = 0;
    // the count's buffer at the size the mark wants it (not grown a second time there); the maximum comes through its first word
    if ((n && (rc = h->f_count.ensure(sizeof(unsigned long long)))) || (rc = labels_max_dev(h, h->f_count, n, d_labels, &mx)))
        return rc;
    return set_slot_core(h, slot, n, d_labels, mx, mode);
}

int ivfhnsw_gpu_clear_filter_slot(ivfhnsw_gpu *h, int slot)
{
    int rc = filter_state(h, "clear_filter_slot");
    if (rc)
        return rc;
    if (slot < -1 || slot >= IVFHNSW_FILTER_SLOTS)
        return fail(IVFHNSW_ERR_INVALID, "clear_filter_slot: slot %d, a handle has slots 0..%d (-1: every slot)", slot,
                    IVFHNSW_FILTER_SLOTS - 1);
    if (slot >= 0 && h->slots[slot].mode < 0)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // searches in flight still read the planes (a split batch joins this stream)
    if (slot < 0) {
        slots_drop(h);
        return IVFHNSW_OK;
    }
    // planes reach to the highest slot in use: clearing that one gives the planes above the next back
    uint32_t np = 0;
    for (int s = 0; s < IVFHNSW_FILTER_SLOTS; s++)
        if (s != slot && h->slots[s].mode >= 0)
            np = (uint32_t)s + 1;
    const size_t pb = (size_t)slot_plane_stride(h->n_local) * sizeof(uint32_t);
    if (np < h->fs.nplanes) {
        ScopedBuf planes;
        if (np && (rc = planes_resized(h, np, planes)))
            return rc;
        HIP_TRY(hipStreamSynchronize(h->stream));
        planes_install(h, planes, np);
    } else {
        HIP_TRY(hipMemsetAsync(h->fs_planes.as<char>() + (size_t)slot * pb, 0, pb, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    h->slots[slot].drop();
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_filter_slot_info(ivfhnsw_gpu *h, unsigned slot, int *mode, uint64_t *rows_passing, uint64_t *rows_total)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    if (slot >= IVFHNSW_FILTER_SLOTS)
        return fail(IVFHNSW_ERR_INVALID, "filter_slot_info: slot %u, a handle has slots 0..%d", slot, IVFHNSW_FILTER_SLOTS - 1);
    const LabelSet &s = (h->is_view && h->parent ? h->parent : h)->slots[slot];
    return label_set_info(s.mode, s.pass, 0, h->n_local, mode, rows_passing, rows_total);
}

// ---- row tags

int ivfhnsw_gpu_set_tags(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, const uint16_t *tags)
{
    int rc = filter_state(h, "set_tags", true, "row tags");
    if (rc || (rc = tags_args(n, labels, tags, "set_tags")))
        return rc;
    ScopedBuf stage_l, stage_t; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_from_host(h, n, labels, stage_l, &mx)) || (n && (rc = stage_in(h, stage_t, tags, n * sizeof(uint16_t)))))
        return rc;
    return set_tags_core(h, n, stage_l.as<uint32_t>(), stage_t.as<uint16_t>(), mx);
}

int ivfhnsw_gpu_set_tags_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, const uint16_t *d_tags)
{
    int rc = filter_state(h, "set_tags_dev", true, "row tags");
    if (rc || (rc = tags_args(n, d_labels, d_tags, "set_tags_dev")))
        return rc;
    if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_tags & 1))
        return fail(IVFHNSW_ERR_INVALID, "set_tags_dev: labels must be 4-byte aligned and tags 2-byte aligned");
    ScopedBuf word; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_max_dev(h, word, n, d_labels, &mx)))
        return rc;
    return set_tags_core(h, n, d_labels, d_tags, mx);
}

int ivfhnsw_gpu_clear_tags(ivfhnsw_gpu *h)
{
    int rc = filter_state(h, "clear_tags", false, "row tags");
    if (rc)
        return rc;
    if (!h->tg_labels)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // searches in flight still read the row tags (a split batch joins this stream)
    tags_drop(h);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_tags_info(ivfhnsw_gpu *h, uint64_t *rows_tagged, uint64_t *rows_total, uint64_t *table_labels)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (rows_tagged && (rc = tags_count(h, IVFHNSW_TAG_NONE, false, rows_tagged)))
        return rc;
    if (rows_total)
        *rows_total = h->n_local;
    if (table_labels)
        *table_labels = h->tg_labels;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_tag_rows(ivfhnsw_gpu *h, unsigned tag, uint64_t *rows)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (tag > IVFHNSW_TAG_NONE || !rows)
        return fail(IVFHNSW_ERR_INVALID, "tag_rows: tag %u (tags are 0..0xffff) or a null result", tag);
    return tags_count(h, tag, true, rows);
}

// ---- row values

int ivfhnsw_gpu_set_values(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, const uint32_t *values)
{
    int rc = filter_state(h, "set_values", true, "row values");
    if (rc || (rc = values_args(n, labels, values, "set_values")))
        return rc;
    ScopedBuf stage_l, stage_v; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_from_host(h, n, labels, stage_l, &mx)) || (n && (rc = stage_in(h, stage_v, values, n * sizeof(uint32_t)))))
        return rc;
    return set_values_core(h, n, stage_l.as<uint32_t>(), stage_v.as<uint32_t>(), mx);
}

int ivfhnsw_gpu_set_values_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, const uint32_t *d_values)
{
    int rc = filter_state(h, "set_values_dev", true, "row values");
    if (rc || (rc = values_args(n, d_labels, d_values, "set_values_dev")))
        return rc;
    if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_values & 3))
        return fail(IVFHNSW_ERR_INVALID, "set_values_dev: labels and values must be 4-byte aligned");
    ScopedBuf word; // of this call only
    uint32_t mx = 0;
    if ((rc = labels_max_dev(h, word, n, d_labels, &mx)))
        return rc;
    return set_values_core(h, n, d_labels, d_values, mx);
}

int ivfhnsw_gpu_clear_values(ivfhnsw_gpu *h)
{
    int rc = filter_state(h, "clear_values", false, "row values");
    if (rc)
        return rc;
    if (!h->vl_labels)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // searches in flight still read the row values (a split batch joins this stream)
    values_drop(h);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_values_info(ivfhnsw_gpu *h, uint64_t *rows_valued, uint64_t *rows_total, uint64_t *table_labels)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (rows_valued && (rc = values_count(h, 0, IVFHNSW_VALUE_NONE - 1, rows_valued)))
        return rc;
    if (rows_total)
        *rows_total = h->n_local;
    if (table_labels)
        *table_labels = h->vl_labels;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_value_rows(ivfhnsw_gpu *h, uint32_t lo, uint32_t hi, uint64_t *rows)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!rows)
        return fail(IVFHNSW_ERR_INVALID, "value_rows: a null result");
    return values_count(h, lo, hi, rows);
}

// ---- row tags AND row values

int ivfhnsw_gpu_tag_value_rows(ivfhnsw_gpu *h, unsigned tag, uint32_t lo, uint32_t hi, uint64_t *rows)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (tag > IVFHNSW_TAG_NONE || !rows)
        return fail(IVFHNSW_ERR_INVALID, "tag_value_rows: tag %u (tags are 0..0xffff) or a null result", tag);
    return tag_values_count(h, tag, lo, hi, rows);
}
