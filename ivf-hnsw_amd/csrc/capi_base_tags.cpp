// Base tags: one uint16 per row of a handle's store, the ground truth of the index's row tags (3.21).  An
// exact _tags call (capi_exact.cpp) answers every query as the plain call would with set_base_filter({rows that carry the
// query's tag}, ALLOW) installed.  The holder keeps the tag of every row and, behind it, the tagged row numbers ordered
// by (tag, row) with their starts per tag: a tag's rows are an ascending list, which is what the Indirect column map
// sweeps (sweep_steps.h).  Both are rebuilt by every set call -- a stable sort of the row numbers by tag.  Independent of
// the base filter, of its slots and of the index's row tags (capi_filter.cpp), whose labels are ids.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

void base_tags_drop(ivfhnsw_gpu *h)
{
    h->bt_tagged = 0;
    h->bt_in_use = 0;
    h->bt_max_rows = 0;
    h->bt_tags.release();
    h->bt_rows.release();
    h->bt_off.release();
}

int base_tags_call(const ivfhnsw_gpu *b, const char *who, TagRows *tr, size_t *tags_in_use)
{
    if (b->bf_mode >= 0)
        return fail(IVFHNSW_ERR_STATE, "%s: the store has a set_base_filter filter installed; a call is filtered by that or by "
                                       "tags, not both (clear_base_filter first)", who);
    *tr = TagRows{};
    tr->n = (uint32_t)b->base_n;
    *tags_in_use = 0;
    if (b->bt_tags.p) {
        tr->off = b->bt_off.as<uint32_t>();
        tr->rows = b->bt_rows.as<uint32_t>();
        *tags_in_use = b->bt_in_use;
    }
    return IVFHNSW_OK;
}

static int base_tags_args(size_t n, const uint32_t *rows, const uint16_t *tags, const char *who)
{
    if (n && (!rows || !tags))
        return fail(IVFHNSW_ERR_INVALID, "%s: null rows or tags", who);
    return IVFHNSW_OK;
}

// d_rows / d_tags [n] in device memory.  The new tag array (the installed one's entries, or untagged, then the n tags
// scattered in), the row lists and their starts are built beside the installed ones and swapped in when nothing can fail
// any more.  A row given two different tags keeps one of them, which the check behind the scatter finds.
static int set_base_tags_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_rows, const uint16_t *d_tags)
{
    if (n == 0)
        return IVFHNSW_OK;
    const uint64_t N = h->base_n;
    ScopedBuf tags, rows, off, work; // work: of this call only
    int rc;
    // work: the conflict word and the two statistics; the sort's keys, its two permutations and its histograms
    const size_t hist_words = 256 * ((N + kKmeansTile - 1) / kKmeansTile);
    if ((rc = tags.ensure(N * sizeof(uint16_t))) || (rc = off.ensure((kTagValues + 1) * sizeof(uint32_t))) ||
        (rc = work.ensure((4 + 3 * N + hist_words) * sizeof(uint32_t))))
        return rc;
    if (h->bt_tags.p)
        HIP_TRY(hipMemcpyAsync(tags.p, h->bt_tags.p, N * sizeof(uint16_t), hipMemcpyDeviceToDevice, h->stream));
    else // 0xffff: IVFHNSW_TAG_NONE
        HIP_TRY(hipMemsetAsync(tags.p, 0xff, N * sizeof(uint16_t), h->stream));
    uint32_t *word = work.as<uint32_t>(), *stats = word + 1, *keys = word + 4, *ids_a = keys + N, *ids_b = ids_a + N, *hist = ids_b + N;
    uint32_t conflict = 0;
    HIP_TRY(launch_base_tags_apply(h->stream, d_rows, d_tags, n, N, tags.as<uint16_t>(), word));
    HIP_TRY(hipMemcpyAsync(&conflict, word, sizeof(conflict), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (conflict)
        return fail(IVFHNSW_ERR_INVALID, "set_base_tags: a row is given two different tags in one call");
    uint32_t *sorted = nullptr;
    HIP_TRY(launch_base_tags_index(h->stream, tags.as<uint16_t>(), N, keys, ids_a, ids_b, hist, off.as<uint32_t>(), stats, &sorted));
    // the words that come back: the tagged rows (the size of the list), the tags in use (the strip bound) and the longest list
    uint32_t st[2] = {0, 0}, tagged = 0;
    HIP_TRY(hipMemcpyAsync(st, stats, sizeof(st), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&tagged, off.as<uint32_t>() + kTagNone, sizeof(tagged), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (tagged) {
        if ((rc = rows.ensure((size_t)tagged * sizeof(uint32_t))))
            return rc;
        HIP_TRY(hipMemcpyAsync(rows.p, sorted, (size_t)tagged * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream)); // the list is complete; exact calls in flight still read the earlier arrays
    tags.install(h->bt_tags); // the earlier arrays go with this scope
    rows.install(h->bt_rows);
    off.install(h->bt_off);
    h->bt_tagged = tagged;
    h->bt_in_use = st[0];
    h->bt_max_rows = st[1];
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_set_base_tags(ivfhnsw_gpu *h, size_t n, const uint32_t *rows, const uint16_t *tags)
{
    int rc = filter_holder_guard(h, kBaseFilter, "set_base_tags", true);
    if (rc || (rc = base_tags_args(n, rows, tags, "set_base_tags")))
        return rc;
    ScopedBuf stage_r, stage_t; // of this call only
    if (n && ((rc = stage_in(h, stage_r, rows, n * sizeof(uint32_t))) || (rc = stage_in(h, stage_t, tags, n * sizeof(uint16_t)))))
        return rc;
    return set_base_tags_core(h, n, stage_r.as<uint32_t>(), stage_t.as<uint16_t>());
}

int ivfhnsw_gpu_set_base_tags_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_rows, const uint16_t *d_tags)
{
    int rc = filter_holder_guard(h, kBaseFilter, "set_base_tags_dev", true);
    if (rc || (rc = base_tags_args(n, d_rows, d_tags, "set_base_tags_dev")))
        return rc;
    if (((uintptr_t)d_rows & 3) || ((uintptr_t)d_tags & 1))
        return fail(IVFHNSW_ERR_INVALID, "set_base_tags_dev: rows must be 4-byte aligned and tags 2-byte aligned");
    return set_base_tags_core(h, n, d_rows, d_tags);
}

int ivfhnsw_gpu_clear_base_tags(ivfhnsw_gpu *h)
{
    int rc = filter_holder_guard(h, kBaseFilter, "clear_base_tags", false);
    if (rc)
        return rc;
    if (!h->bt_tags.p)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // exact calls in flight still read the lists
    base_tags_drop(h);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_base_tags_info(ivfhnsw_gpu *h, uint64_t *rows_tagged, uint64_t *rows_total, uint64_t *tags_in_use)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    if (rows_tagged)
        *rows_tagged = b->bt_tagged;
    if (rows_total)
        *rows_total = b->base_n;
    if (tags_in_use)
        *tags_in_use = b->bt_in_use;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_base_tag_rows(ivfhnsw_gpu *h, unsigned tag, uint64_t *rows)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (tag > IVFHNSW_TAG_NONE || !rows)
        return fail(IVFHNSW_ERR_INVALID, "base_tag_rows: tag %u (tags are 0..0xffff) or a null result", tag);
    const ivfhnsw_gpu *b = h->parent ? h->parent : h;
    if (!b->base_n)
        return fail(IVFHNSW_ERR_STATE, "base_tag_rows before upload_base");
    if (!b->bt_tags.p) { // no tag array: every row is untagged
        *rows = tag == IVFHNSW_TAG_NONE ? b->base_n : 0;
        return IVFHNSW_OK;
    }
    // off[kTagValues] = the rows of the store: "none" reads like any tag
    uint32_t lim[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(lim, b->bt_off.as<uint32_t>() + tag, sizeof(lim), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *rows = lim[1] - lim[0];
    return IVFHNSW_OK;
}
