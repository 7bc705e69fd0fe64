#include "capi_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// searchDisk's exact re-rank on the device (IndexIVF_HNSW_Grouping.cpp:365-395): the base store and the re-rank itself.

// rows [first, first + count) of the store from `rows` at row_stride (device memory when on_device); first == 0
// (re)allocates the store, n == 0 frees it.  Synchronous: the caller may reuse `rows` when it returns.
static int upload_base_impl(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const uint8_t *rows,
                            size_t row_stride, bool on_device)
{
    int rc = table_change_guard(h, kUploads, "upload_base", false);
    if (rc)
        return rc;
    if (n == 0) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->base_rows.release();
        h->base_stage.release();
        base_filter_drop(h); // its rows are gone
        base_slots_drop(h);
        base_tags_drop(h);
        base_values_drop(h);
        h->base_n = 0;
        h->base_d = 0;
        return IVFHNSW_OK;
    }
    if (d % 16 || d < 16 || d > 512)
        return fail(IVFHNSW_ERR_INVALID, "base dimension %zu: must be a multiple of 16 in 16..512", d);
    if (n >= 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "base of %zu rows: labels must fit 32 bits", n);
    if (first > n || count > n - first)
        return fail(IVFHNSW_ERR_INVALID, "rows [%zu, %zu) outside a base of %zu rows", first, first + count, n);
    if (count && (!rows || row_stride < d))
        return fail(IVFHNSW_ERR_INVALID, "null rows or row_stride %zu < d %zu", row_stride, d);
    if (first == 0) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        h->base_rows.release();
        base_filter_drop(h); // a new store: its row numbers mean other rows
        base_slots_drop(h);
        base_tags_drop(h);
        base_values_drop(h);
        h->base_n = 0;
        h->base_d = 0;
        if ((rc = h->base_rows.ensure(n * d)))
            return fail(rc, "base store of %zu x %zu bytes: %s", n, d, ivfhnsw_gpu_last_error());
        HIP_TRY(hipMemsetAsync(h->base_rows.p, 0, n * d, h->stream));
        h->base_n = n;
        h->base_d = d;
    } else if (!h->base_n) {
        return fail(IVFHNSW_ERR_STATE, "upload_base with first = %zu: no store (the first call has first = 0)", first);
    } else if (h->base_n != n || h->base_d != d) {
        return fail(IVFHNSW_ERR_INVALID, "upload_base: store holds %llu x %zu, call says %zu x %zu",
                    (unsigned long long)h->base_n, h->base_d, n, d);
    }
    uint8_t *dst = h->base_rows.as<uint8_t>() + first * d;
    if (on_device) {
        HIP_TRY(launch_rerank_permute(h->stream, rows, row_stride, dst, count, (int)d));
    } else {
        // host rows in pieces of at most 64 MB through a device staging buffer
        const size_t chunk = std::max<size_t>(1, ((size_t)64 << 20) / d);
        if (count && (rc = h->base_stage.ensure(std::min(chunk, count) * d)))
            return rc;
        for (size_t r0 = 0; r0 < count; r0 += chunk) {
            const size_t m = std::min(chunk, count - r0);
            HIP_TRY(hipMemcpy2DAsync(h->base_stage.p, d, rows + r0 * row_stride, row_stride, d, m, hipMemcpyHostToDevice,
                                     h->stream));
            HIP_TRY(launch_rerank_permute(h->stream, h->base_stage.as<uint8_t>(), d, dst + r0 * d, m, (int)d));
        }
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_upload_base(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const uint8_t *rows,
                            size_t row_stride)
{
    return upload_base_impl(h, n, d, first, count, rows, row_stride, false);
}

int ivfhnsw_gpu_upload_base_dev(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const uint8_t *d_rows,
                                size_t row_stride)
{
    return upload_base_impl(h, n, d, first, count, d_rows, row_stride, true);
}

// the handle that holds the store: a view reads its parent's
static const ivfhnsw_gpu *base_holder(const ivfhnsw_gpu *h) { return h->parent ? h->parent : h; }

static int check_rerank(ivfhnsw_gpu *h, size_t kc, size_t k)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!base_holder(h)->base_n)
        return fail(IVFHNSW_ERR_STATE, "rerank before upload_base");
    if (k < 1 || k > kc || kc > 4096)
        return fail(IVFHNSW_ERR_INVALID, "rerank needs 1 <= k <= kc <= 4096 (k %zu, kc %zu)", k, kc);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_rerank_dev(ivfhnsw_gpu *h, size_t nq, size_t kc, const float *d_queries, const int64_t *d_cand, size_t k,
                           float *d_distances, int64_t *d_labels)
{
    int rc = check_rerank(h, kc, k);
    if (rc)
        return rc;
    if (nq == 0)
        return IVFHNSW_OK;
    if (!d_queries || !d_cand || !d_distances || !d_labels)
        return fail(IVFHNSW_ERR_INVALID, "null query/candidate/result buffer");
    const ivfhnsw_gpu *b = base_holder(h);
    HIP_TRY(launch_rerank(h->stream, b->base_rows.as<uint8_t>(), b->base_n, (int)b->base_d, d_queries, d_cand, nq, (int)kc,
                          (int)k, d_distances, d_labels));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_rerank(ivfhnsw_gpu *h, size_t nq, size_t kc, const float *queries, const int64_t *cand, size_t k,
                       float *distances, int64_t *labels)
{
    int rc = check_rerank(h, kc, k);
    if (rc)
        return rc;
    if (nq == 0)
        return IVFHNSW_OK;
    if (!queries || !cand || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "null query/candidate/result buffer");
    const ivfhnsw_gpu *b = base_holder(h);
    const int64_t n = (int64_t)b->base_n;
    for (size_t i = 0; i < nq * kc; i++)
        if (cand[i] < -1 || cand[i] >= n)
            return fail(IVFHNSW_ERR_INVALID, "candidate %zu of query %zu is label %lld, outside [-1, %lld)", i % kc, i / kc,
                        (long long)cand[i], (long long)n);
    const size_t d = b->base_d;
    if ((rc = h->r_q.ensure(nq * d * sizeof(float))) || (rc = h->r_cand.ensure(nq * kc * sizeof(int64_t))) ||
        (rc = h->r_dist.ensure(nq * k * sizeof(float))) || (rc = h->r_lab.ensure(nq * k * sizeof(int64_t))))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->r_q.p, queries, nq * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->r_cand.p, cand, nq * kc * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_rerank(h->stream, b->base_rows.as<uint8_t>(), b->base_n, (int)d, h->r_q.as<float>(),
                          h->r_cand.as<int64_t>(), nq, (int)kc, (int)k, h->r_dist.as<float>(), h->r_lab.as<int64_t>()));
    HIP_TRY(hipMemcpyAsync(distances, h->r_dist.p, nq * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(labels, h->r_lab.p, nq * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}
