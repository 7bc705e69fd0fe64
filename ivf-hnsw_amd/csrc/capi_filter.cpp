// The label filter of a handle: searches return only rows whose id is in an allowed set, or is not in a
// denied one.  The set becomes a bitmap over [0, max label], the bitmap one PASS bit per resident row, and the filtered
// forms of the scan kernels read that bit beside the row's norm code.  The bitmap stays with the handle so that in-place
// updates can judge the rows of their new arrays (ListArrays::mark_filter, capi_internal.h).
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
    return mark_rows(h, ids, n_local, h->f_has_bits ? h->f_bits.as<uint32_t>() : nullptr, h->f_max_label, h->filter_mode, mask,
                     pass);
}

void filter_drop(ivfhnsw_gpu *h)
{
    h->filter_mode = -1;
    h->fmask = nullptr;
    h->f_has_bits = false;
    h->f_max_label = 0;
    h->f_pass = 0;
    h->f_mask.release();
    h->f_bits.release();
}

static int filter_state(ivfhnsw_gpu *h, const char *who)
{
    if (h && h->is_view)
        return fail(IVFHNSW_ERR_STATE, "%s: a filter goes to the handle that holds the tables, not to a view of it", who);
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_ivf", who);
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle is shard %u of %u; sharded handles have no label filter", who,
                    h->t.shard_rank, h->t.shard_world);
    return IVFHNSW_OK;
}

// d_labels [n] in device memory (n > 0: max_label = their maximum), read on the handle's stream.  The new bitmap and mask
// are built beside the installed ones and swapped in when complete: any error leaves the earlier filter in force.
static int set_filter_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, int mode)
{
    DevBuf bits, mask;
    int rc = IVFHNSW_OK;
    uint64_t pass = 0;
    if (n && (rc = bits.ensure(((size_t)max_label / 32 + 1) * sizeof(uint32_t))) == IVFHNSW_OK) {
        hipError_t e = launch_remove_bits(h->stream, d_labels, n, max_label, bits.as<uint32_t>());
        if (e != hipSuccess)
            rc = fail(IVFHNSW_ERR_HIP, "set_filter: %s", hipGetErrorString(e));
    }
    if (rc == IVFHNSW_OK)
        rc = mark_rows(h, h->t.ids, h->n_local, n ? bits.as<uint32_t>() : nullptr, max_label, mode, mask, &pass);
    if (rc) {
        bits.release();
        mask.release();
        return rc;
    }
    std::swap(h->f_bits, bits);
    std::swap(h->f_mask, mask);
    bits.release(); // the earlier filter's
    mask.release();
    h->filter_mode = mode;
    h->fmask = h->f_mask.as<uint32_t>();
    h->f_has_bits = n != 0;
    h->f_max_label = n ? max_label : 0;
    h->f_pass = pass;
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

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_set_filter(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode)
{
    int rc = filter_state(h, "set_filter");
    if (rc || (rc = check_args(n, labels, mode, "set_filter")))
        return rc;
    uint32_t mx = 0;
    for (size_t i = 0; i < n; i++)
        mx = std::max(mx, labels[i]);
    if (n) {
        if ((rc = h->f_labels.ensure(n * sizeof(uint32_t))))
            return rc;
        HIP_TRY(hipMemcpyAsync(h->f_labels.p, labels, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    }
    rc = set_filter_core(h, n, h->f_labels.as<uint32_t>(), mx, mode);
    h->f_labels.release(); // staging of this call only
    return rc;
}

int ivfhnsw_gpu_set_filter_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int mode)
{
    int rc = filter_state(h, "set_filter_dev");
    if (rc || (rc = check_args(n, d_labels, mode, "set_filter_dev")))
        return rc;
    if ((uintptr_t)d_labels & 3)
        return fail(IVFHNSW_ERR_INVALID, "set_filter_dev: labels must be 4-byte aligned");
    uint32_t mx = 0;
    if (n) {
        if ((rc = h->f_count.ensure(sizeof(unsigned long long))))
            return rc;
        HIP_TRY(hipMemsetAsync(h->f_count.p, 0, sizeof(uint32_t), h->stream));
        HIP_TRY(launch_remove_max(h->stream, d_labels, n, h->f_count.as<uint32_t>()));
        HIP_TRY(hipMemcpyAsync(&mx, h->f_count.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    return set_filter_core(h, n, d_labels, mx, mode);
}

int ivfhnsw_gpu_clear_filter(ivfhnsw_gpu *h)
{
    if (h && h->is_view)
        return fail(IVFHNSW_ERR_STATE, "clear_filter: a filter goes to the handle that holds the tables, not to a view of it");
    int rc = bind(h);
    if (rc)
        return rc;
    if (h->filter_mode < 0)
        return IVFHNSW_OK;
    HIP_TRY(hipStreamSynchronize(h->stream)); // searches in flight still read the mask (a split batch joins this stream)
    filter_drop(h);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_filter_info(ivfhnsw_gpu *h, int *mode, uint64_t *rows_passing, uint64_t *rows_total)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    if (mode)
        *mode = h->filter_mode;
    if (rows_passing)
        *rows_passing = h->filter_mode >= 0 ? h->f_pass : h->n_local;
    if (rows_total)
        *rows_total = h->n_local;
    return IVFHNSW_OK;
}
