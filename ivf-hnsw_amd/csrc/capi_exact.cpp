#include "capi_internal.h"

// ---------------------------------------------------------------------------------------------------------------------
// Exact brute-force search of the uint8 base store (kernels_exact.hip): the ground truth the drivers
// read as -path_gt (tests/test_ivfhnsw_sift1b.cpp:173-215), computed from the store upload_base left in HBM.

namespace {

// queries per pass of the kernel: bounds the permuted queries and, with the splits, the partial tables (<= 256 MB)
constexpr size_t kExactChunk = 16384;
constexpr size_t kExactPartBytes = (size_t)256 << 20;

int exact_impl(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k, float *distances,
               int64_t *labels, bool on_device)
{
    int rc = bind(h);
    if (rc)
        return rc;
    const ivfhnsw_gpu *b = h->parent ? h->parent : h; // a view searches its parent's store
    if (!b->base_n)
        return fail(IVFHNSW_ERR_STATE, "exact_search before upload_base");
    const size_t d = b->base_d, n = b->base_n;
    if (d > 256)
        return fail(IVFHNSW_ERR_INVALID,
                    "exact_search on a store of dimension %zu: beyond d = 256 the squared distance can exceed 2^24 and is no "
                    "longer the exact float fvec_L2sqr returns",
                    d);
    if (k < 1 || k > 100)
        return fail(IVFHNSW_ERR_INVALID, "exact_search needs 1 <= k <= 100 (k %zu)", k);
    if (nq == 0)
        return IVFHNSW_OK;
    if (!queries || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "null query/result buffer");
    if (row_stride < d)
        return fail(IVFHNSW_ERR_INVALID, "row_stride %zu < d %zu", row_stride, d);

    const size_t first = std::min(nq, kExactChunk);
    const int nsplit = h->opt_exact_splits > 0 ? h->opt_exact_splits : exact_splits_for(first, n, (int)k);
    size_t chunk = kExactPartBytes / ((size_t)nsplit * k * sizeof(uint64_t));
    chunk = std::max<size_t>(128, std::min(kExactChunk, chunk / 128 * 128));
    chunk = std::min(chunk, nq);
    if ((rc = h->ex_q.ensure(chunk * d)) || (rc = h->ex_part.ensure((size_t)nsplit * chunk * k * sizeof(uint64_t))))
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
        // the queries in the store's byte order: an integer sum does not care which order, only that it is the same
        HIP_TRY(launch_rerank_permute(h->stream, src, src_stride, h->ex_q.as<uint8_t>(), m, (int)d));
        float *od = on_device ? distances + q0 * k : h->ex_dist.as<float>();
        int64_t *ol = on_device ? labels + q0 * k : h->ex_lab.as<int64_t>();
        HIP_TRY(launch_exact_search(h->stream, h->ex_q.as<uint8_t>(), b->base_rows.as<uint8_t>(), m, n, (int)d, (int)k, nsplit,
                                    h->ex_part.as<unsigned long long>(), od, ol));
        if (!on_device) {
            HIP_TRY(hipMemcpyAsync(distances + q0 * k, od, m * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipMemcpyAsync(labels + q0 * k, ol, m * k * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
            // the next chunk reuses the pageable source and the staging buffers
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
    }
    return IVFHNSW_OK;
}

} // namespace

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
