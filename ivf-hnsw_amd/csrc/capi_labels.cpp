// What the calls that take a set of uint32 labels share: the filter, the filter slots and the base
// filter, removal, locate and reconstruct by label.  The labels come in host or device memory and become, with removal's
// kernels (kernels_remove.hip), a device bitmap over [0, largest label]; what each call does with the bitmap is its own.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

int run_with_word(ivfhnsw_gpu *h, DevBuf &word, int init, const std::function<hipError_t(uint32_t *)> &launch, uint32_t *out)
{
    int rc;
    if ((rc = word.ensure(sizeof(uint32_t))))
        return rc;
    HIP_TRY(hipMemsetAsync(word.p, init, sizeof(uint32_t), h->stream));
    HIP_TRY(launch(word.as<uint32_t>()));
    HIP_TRY(hipMemcpyAsync(out, word.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int label_args_guard(size_t n, const uint32_t *labels, const char *who, const int *mode)
{
    if (n && !labels)
        return fail(IVFHNSW_ERR_INVALID, "%s: null labels", who);
    if (mode && *mode != IVFHNSW_FILTER_ALLOW && *mode != IVFHNSW_FILTER_DENY)
        return fail(IVFHNSW_ERR_INVALID, "%s: mode %d is neither IVFHNSW_FILTER_ALLOW nor IVFHNSW_FILTER_DENY", who, *mode);
    return IVFHNSW_OK;
}

int labels_from_host(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, DevBuf &stage, uint32_t *max_label)
{
    if (max_label) {
        uint32_t mx = 0;
        for (size_t i = 0; i < n; i++)
            mx = std::max(mx, labels[i]);
        *max_label = mx;
    }
    return n ? stage_in(h, stage, labels, n * sizeof(uint32_t)) : IVFHNSW_OK;
}

int labels_max_dev(ivfhnsw_gpu *h, DevBuf &word, size_t n, const uint32_t *d_labels, uint32_t *max_label)
{
    *max_label = 0;
    if (n == 0)
        return IVFHNSW_OK;
    return run_with_word(h, word, 0, [&](uint32_t *out) { return launch_remove_max(h->stream, d_labels, n, out); }, max_label);
}

int labels_bitmap(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, DevBuf &bits)
{
    if (n == 0)
        return IVFHNSW_OK;
    int rc = bits.ensure(label_bitmap_words(max_label) * sizeof(uint32_t));
    if (rc)
        return rc;
    HIP_TRY(launch_remove_bits(h->stream, d_labels, n, max_label, bits.as<uint32_t>()));
    return IVFHNSW_OK;
}

int filter_holder_guard(ivfhnsw_gpu *h, FilterKind kind, const char *who, bool need_upload)
{
    const bool base = kind == kBaseFilter;
    if (h && h->is_view)
        return fail(IVFHNSW_ERR_STATE, "%s: a %s goes to the handle that holds the %s, not to a view of it", who,
                    base ? "base filter" : "filter", base ? "store" : "tables");
    int rc = bind(h);
    if (rc)
        return rc;
    if (need_upload && !(base ? h->base_n != 0 : h->has_ivf))
        return fail(IVFHNSW_ERR_STATE, "%s before %s", who, base ? "upload_base" : "upload_ivf");
    return IVFHNSW_OK;
}

int label_set_info(int set_mode, uint64_t pass, uint64_t unset_pass, uint64_t total, int *mode, uint64_t *rows_passing,
                   uint64_t *rows_total)
{
    if (mode)
        *mode = set_mode;
    if (rows_passing)
        *rows_passing = set_mode >= 0 ? pass : unset_pass;
    if (rows_total)
        *rows_total = total;
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl
