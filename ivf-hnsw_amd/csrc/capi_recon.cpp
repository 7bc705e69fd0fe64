// Reconstruction of stored vectors: faiss's reconstruct / reconstruct_n / search_and_reconstruct and the
// label -> row lookup of its direct map, for the lists the handle holds.  Read-only: the tables, the filter and the range
// results of the handle stay as they are; search_reconstruct leaves the plan its search left.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

// rows of one launch chain where a chunk is staged: the ROTATED vectors of an OPQ index on their way through launch_opq
// (rc_y), and the output of the host-pointer forms (rc_out)
static constexpr size_t kReconChunk = (size_t)1 << 18;

static int recon_state(ivfhnsw_gpu *h, const char *who, bool need_quantizer)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_ivf", who);
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle is shard %u of %u; a shard holds only its own lists", who, h->t.shard_rank,
                    h->t.shard_world);
    if (!need_quantizer)
        return IVFHNSW_OK;
    if (!h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_quantizer (the centroids are the quantizer's vectors)", who);
    if (h->gr.d != h->t.d || h->gr.n != h->t.nc)
        return fail(IVFHNSW_ERR_STATE, "%s: quantizer (%u x %d) does not match the index (%u x %d)", who, h->gr.n, h->gr.d, h->t.nc,
                    h->t.d);
    return IVFHNSW_OK;
}

static int check_space(int space, const char *who)
{
    if (space != IVFHNSW_RECON_ORIGINAL && space != IVFHNSW_RECON_ROTATED)
        return fail(IVFHNSW_ERR_INVALID, "%s: space %d is neither IVFHNSW_RECON_ORIGINAL nor IVFHNSW_RECON_ROTATED", who, space);
    return IVFHNSW_OK;
}

// d_rows [n] -> d_out [n][d], device pointers, asynchronous on the handle's stream
static int recon_rows_core(ivfhnsw_gpu *h, size_t n, const int64_t *d_rows, int space, float *d_out)
{
    const GroupTables *g = h->has_group ? &h->g : nullptr;
    const size_t d = (size_t)h->t.d;
    if (space == IVFHNSW_RECON_ROTATED || !h->opq_A) {
        hipError_t e = launch_recon_rows(h->stream, h->t, g, h->gr.vectors, h->n_local, d_rows, n, d_out);
        if (e == hipErrorInvalidValue)
            return fail(IVFHNSW_ERR_INVALID, "reconstruct: %zu rows in one call is more than the kernel takes", n);
        HIP_TRY(e);
        return IVFHNSW_OK;
    }
    // x = A^T y: the chunk in ROTATED space, then launch_opq with the matrix as uploaded (transform_transpose's order)
    int rc = h->rc_y.ensure(std::min(n, kReconChunk) * d * sizeof(float));
    if (rc)
        return rc;
    for (size_t i0 = 0; i0 < n; i0 += kReconChunk) {
        const size_t m = std::min(kReconChunk, n - i0);
        HIP_TRY(launch_recon_rows(h->stream, h->t, g, h->gr.vectors, h->n_local, d_rows + i0, m, h->rc_y.as<float>()));
        HIP_TRY(launch_opq(h->stream, h->opq_A, h->rc_y.as<float>(), d_out + i0 * d, (int)m, (int)d));
        HIP_TRY(launch_recon_refill(h->stream, h->n_local, d_rows + i0, m, (int)d, d_out + i0 * d));
    }
    return IVFHNSW_OK;
}

// d_rows [n] (device) -> out [n][d] (host) through rc_out, a chunk at a time; returns with the stream drained
static int recon_rows_to_host(ivfhnsw_gpu *h, size_t n, const int64_t *d_rows, int space, float *out)
{
    const size_t d = (size_t)h->t.d;
    int rc = h->rc_out.ensure(std::min(n, kReconChunk) * d * sizeof(float));
    if (rc)
        return rc;
    for (size_t i0 = 0; i0 < n; i0 += kReconChunk) {
        const size_t m = std::min(kReconChunk, n - i0);
        if ((rc = recon_rows_core(h, m, d_rows + i0, space, h->rc_out.as<float>())))
            return rc;
        HIP_TRY(hipMemcpyAsync(out + i0 * d, h->rc_out.p, m * d * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

// The words locate keeps in lc_scalar; the first is the word labels_max_dev answers through.
struct LocateScalars {
    uint32_t max_label, pad;
    unsigned long long missing;
};
static_assert(offsetof(LocateScalars, max_label) == 0, "labels_max_dev writes the buffer's first word");

// d_labels [n] -> d_rows [n], d_counts [n] (nullable), device pointers on the handle's stream; the requests without a row
// are counted in lc_scalar's `missing`.  Synchronises once (the bitmap is sized by the largest label).
static int locate_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int64_t *d_rows, uint32_t *d_counts)
{
    if (n > 0x7fffffffull)
        return fail(IVFHNSW_ERR_INVALID, "locate: %zu labels in one call (at most 2^31 - 1)", n);
    const size_t nblocks = (n + kKmeansTile - 1) / kKmeansTile;
    int rc;
    if ((rc = h->lc_scalar.ensure(sizeof(LocateScalars))) || (rc = h->lc_perm.ensure(n * sizeof(uint32_t))) ||
        (rc = h->lc_perm2.ensure(n * sizeof(uint32_t))) || (rc = h->lc_hist.ensure(256 * nblocks * sizeof(uint32_t))) ||
        (rc = h->lc_sorted.ensure(n * sizeof(uint32_t))) || (rc = h->lc_lo.ensure(n * sizeof(uint32_t))) ||
        (rc = h->lc_cnt.ensure(n * sizeof(uint32_t))))
        return rc;
    LocateScalars *sc = h->lc_scalar.as<LocateScalars>();
    uint32_t mx = 0;
    HIP_TRY(hipMemsetAsync(sc, 0, sizeof(LocateScalars), h->stream));
    if ((rc = labels_max_dev(h, h->lc_scalar, n, d_labels, &mx)) || (rc = labels_bitmap(h, n, d_labels, mx, h->lc_bits)))
        return rc;
    int key_bits = 1;
    while (key_bits < 32 && (mx >> key_bits))
        key_bits++;
    uint32_t *perm = nullptr;
    HIP_TRY(launch_sort_by_key(h->stream, d_labels, n, key_bits, h->lc_perm.as<uint32_t>(), h->lc_perm2.as<uint32_t>(),
                               h->lc_hist.as<uint32_t>(), &perm));
    uint32_t *sorted = h->lc_sorted.as<uint32_t>(), *lo = h->lc_lo.as<uint32_t>(), *cnt = h->lc_cnt.as<uint32_t>();
    HIP_TRY(launch_locate_gather(h->stream, d_labels, perm, n, sorted));
    HIP_TRY(hipMemsetAsync(lo, 0xff, n * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(cnt, 0, n * sizeof(uint32_t), h->stream));
    HIP_TRY(launch_locate_hit(h->stream, h->t.ids, h->n_local, h->lc_bits.as<uint32_t>(), mx, sorted, n, lo, cnt));
    HIP_TRY(launch_locate_scatter(h->stream, sorted, perm, n, lo, cnt, d_rows, d_counts, &sc->missing));
    return IVFHNSW_OK;
}

// after locate_core: *n_missing (non-null) from the device; returns with the stream drained
static int read_missing(ivfhnsw_gpu *h, uint64_t *n_missing)
{
    unsigned long long miss = 0;
    HIP_TRY(hipMemcpyAsync(&miss, &h->lc_scalar.as<LocateScalars>()->missing, sizeof(miss), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    *n_missing = miss;
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_locate(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int64_t *rows, uint32_t *counts)
{
    int rc = recon_state(h, "locate", false);
    if (rc || n == 0)
        return rc;
    if (!labels || !rows)
        return fail(IVFHNSW_ERR_INVALID, "locate: null labels or rows");
    if ((rc = h->lc_rows.ensure(n * sizeof(int64_t))) || (counts && (rc = h->lc_counts.ensure(n * sizeof(uint32_t)))) ||
        (rc = labels_from_host(h, n, labels, h->lc_labels, nullptr)) ||
        (rc = locate_core(h, n, h->lc_labels.as<uint32_t>(), h->lc_rows.as<int64_t>(), counts ? h->lc_counts.as<uint32_t>() : nullptr)) ||
        (rc = stage_out(h, rows, h->lc_rows, n * sizeof(int64_t))) ||
        (counts && (rc = stage_out(h, counts, h->lc_counts, n * sizeof(uint32_t)))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_locate_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int64_t *d_rows, uint32_t *d_counts)
{
    int rc = recon_state(h, "locate_dev", false);
    if (rc || n == 0)
        return rc;
    if (!d_labels || !d_rows)
        return fail(IVFHNSW_ERR_INVALID, "locate_dev: null labels or rows");
    if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_rows & 7) || ((uintptr_t)d_counts & 3))
        return fail(IVFHNSW_ERR_INVALID, "locate_dev: labels and counts must be 4-byte aligned, rows 8-byte");
    if ((rc = locate_core(h, n, d_labels, d_rows, d_counts)))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_reconstruct_rows(ivfhnsw_gpu *h, size_t n, const int64_t *rows, int space, float *out)
{
    int rc = recon_state(h, "reconstruct_rows", true);
    if (rc || (rc = check_space(space, "reconstruct_rows")) || n == 0)
        return rc;
    if (!rows || !out)
        return fail(IVFHNSW_ERR_INVALID, "reconstruct_rows: null rows or out");
    for (size_t i = 0; i < n; i++)
        if (rows[i] < -1 || rows[i] >= (int64_t)h->n_local)
            return fail(IVFHNSW_ERR_INVALID, "reconstruct_rows: rows[%zu] = %lld is outside [-1, %llu)", i, (long long)rows[i],
                        (unsigned long long)h->n_local);
    if ((rc = stage_in(h, h->rc_rows, rows, n * sizeof(int64_t))))
        return rc;
    return recon_rows_to_host(h, n, h->rc_rows.as<int64_t>(), space, out);
}

int ivfhnsw_gpu_reconstruct_rows_dev(ivfhnsw_gpu *h, size_t n, const int64_t *d_rows, int space, float *d_out)
{
    int rc = recon_state(h, "reconstruct_rows_dev", true);
    if (rc || (rc = check_space(space, "reconstruct_rows_dev")) || n == 0)
        return rc;
    if (!d_rows || !d_out)
        return fail(IVFHNSW_ERR_INVALID, "reconstruct_rows_dev: null rows or out");
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_out & 3))
        return fail(IVFHNSW_ERR_INVALID, "reconstruct_rows_dev: rows must be 8-byte aligned, out 4-byte");
    return recon_rows_core(h, n, d_rows, space, d_out);
}

int ivfhnsw_gpu_reconstruct(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int space, float *out, uint64_t *n_missing)
{
    int rc = recon_state(h, "reconstruct", true);
    if (rc || (rc = check_space(space, "reconstruct")))
        return rc;
    if (n == 0) {
        if (n_missing)
            *n_missing = 0;
        return IVFHNSW_OK;
    }
    if (!labels || !out)
        return fail(IVFHNSW_ERR_INVALID, "reconstruct: null labels or out");
    uint64_t miss = 0;
    if ((rc = h->lc_rows.ensure(n * sizeof(int64_t))) || (rc = labels_from_host(h, n, labels, h->lc_labels, nullptr)) ||
        (rc = locate_core(h, n, h->lc_labels.as<uint32_t>(), h->lc_rows.as<int64_t>(), nullptr)) || (rc = read_missing(h, &miss)) ||
        (rc = recon_rows_to_host(h, n, h->lc_rows.as<int64_t>(), space, out)))
        return rc;
    if (n_missing)
        *n_missing = miss;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_reconstruct_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int space, float *d_out, uint64_t *n_missing)
{
    int rc = recon_state(h, "reconstruct_dev", true);
    if (rc || (rc = check_space(space, "reconstruct_dev")))
        return rc;
    if (n == 0) {
        if (n_missing)
            *n_missing = 0;
        return IVFHNSW_OK;
    }
    if (!d_labels || !d_out)
        return fail(IVFHNSW_ERR_INVALID, "reconstruct_dev: null labels or out");
    if (((uintptr_t)d_labels & 3) || ((uintptr_t)d_out & 3))
        return fail(IVFHNSW_ERR_INVALID, "reconstruct_dev: labels and out must be 4-byte aligned");
    if ((rc = h->lc_rows.ensure(n * sizeof(int64_t))) ||
        (rc = locate_core(h, n, d_labels, h->lc_rows.as<int64_t>(), nullptr)) ||
        (rc = recon_rows_core(h, n, h->lc_rows.as<int64_t>(), space, d_out)))
        return rc;
    return n_missing ? read_missing(h, n_missing) : IVFHNSW_OK;
}

int ivfhnsw_gpu_search_reconstruct_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                       const float *d_coarse_dists, const ivfhnsw_search_params *p, int space,
                                       float *d_distances, int64_t *d_labels, int64_t *d_rows, float *d_recons)
{
    int rc = recon_state(h, "search_reconstruct", true);
    if (rc || (rc = check_space(space, "search_reconstruct")) || (rc = search_args_guard(h, p, k)) || nq == 0)
        return rc;
    if (!d_queries || !d_distances || !d_labels || !d_recons)
        return fail(IVFHNSW_ERR_INVALID, "search_reconstruct: null query/result buffer");
    if (((uintptr_t)d_rows & 7) || ((uintptr_t)d_recons & 3))
        return fail(IVFHNSW_ERR_INVALID, "search_reconstruct: rows must be 8-byte aligned, recons 4-byte");
    const bool heap = p->heap_order && k > 1;
    // search_dev with out_keys takes one slice of the workspace bound per call (its plan has to stay whole)
    const size_t max_nq = heap ? kMaxBatchAll / 8 : kMaxBatchAll, d = (size_t)h->t.d, np = p->nprobe;
    for (size_t q0 = 0; q0 < nq; q0 += max_nq) {
        const size_t n = std::min(max_nq, nq - q0);
        if ((rc = h->sr_keys.ensure(n * k * sizeof(int64_t))) || (!d_rows && (rc = h->sr_rows.ensure(n * k * sizeof(int64_t)))))
            return rc;
        int64_t *keys = h->sr_keys.as<int64_t>(), *rows = d_rows ? d_rows + q0 * k : h->sr_rows.as<int64_t>();
        float *dist = d_distances + q0 * k;
        int64_t *lab = d_labels + q0 * k;
        if ((rc = ivfhnsw_gpu_search_dev(h, n, k, d_queries + q0 * d, d_coarse_ids ? d_coarse_ids + q0 * np : nullptr,
                                         d_coarse_dists ? d_coarse_dists + q0 * np : nullptr, p, dist, lab, keys)))
            return rc;
        // heap order: with out_keys the search leaves the candidate stream and the replay to its caller; the heap array as
        // keys, then distances and labels out of the keys
        if (heap && ((rc = ivfhnsw_gpu_replay_stream_dev(h, n, k, h->w_stream.as<uint64_t>(), h->w_slen.as<uint32_t>(),
                                                         kHeapStreamCap, keys)) ||
                     (rc = ivfhnsw_gpu_resolve_keys_dev(h, n, k, keys, dist, lab))))
            return rc;
        HIP_TRY(launch_resolve_rows(h->stream, plan_of(h, h->last_max_seg, n), keys, (int)k, rows));
        if ((rc = recon_rows_core(h, n * k, rows, space, d_recons + q0 * k * d)))
            return rc;
    }
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_search_reconstruct(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                                   const float *coarse_dists, const ivfhnsw_search_params *p, int space, float *distances,
                                   int64_t *labels, int64_t *rows, float *recons)
{
    int rc = recon_state(h, "search_reconstruct", true);
    if (rc || (rc = check_space(space, "search_reconstruct")) || (rc = search_args_guard(h, p, k)) || nq == 0)
        return rc;
    if (!queries || !distances || !labels || !recons)
        return fail(IVFHNSW_ERR_INVALID, "search_reconstruct: null query/result buffer");
    if ((coarse_ids == nullptr) != (coarse_dists == nullptr))
        return fail(IVFHNSW_ERR_INVALID, "coarse_ids and coarse_dists must both be given or both be NULL");
    // slices of at most kReconChunk results, so that the staging of the reconstructions stays bounded
    const size_t d = (size_t)h->t.d, np = p->nprobe, step = std::max<size_t>(1, kReconChunk / k);
    for (size_t q0 = 0; q0 < nq; q0 += step) {
        const size_t n = std::min(step, nq - q0), in_c = n * np * sizeof(uint32_t);
        if ((rc = h->s_dist.ensure(n * k * sizeof(float))) || (rc = h->s_lab.ensure(n * k * sizeof(int64_t))) ||
            (rc = h->sr_rows.ensure(n * k * sizeof(int64_t))) || (rc = h->rc_out.ensure(n * k * d * sizeof(float))) ||
            (rc = stage_in(h, h->s_q, queries + q0 * d, n * d * sizeof(float))) ||
            (coarse_ids && ((rc = stage_in(h, h->s_cid, coarse_ids + q0 * np, in_c)) ||
                            (rc = stage_in(h, h->s_cd, coarse_dists + q0 * np, in_c)))) ||
            (rc = ivfhnsw_gpu_search_reconstruct_dev(h, n, k, h->s_q.as<float>(), coarse_ids ? h->s_cid.as<uint32_t>() : nullptr,
                                                     coarse_ids ? h->s_cd.as<float>() : nullptr, p, space, h->s_dist.as<float>(),
                                                     h->s_lab.as<int64_t>(), h->sr_rows.as<int64_t>(), h->rc_out.as<float>())) ||
            (rc = stage_out(h, distances + q0 * k, h->s_dist, n * k * sizeof(float))) ||
            (rc = stage_out(h, labels + q0 * k, h->s_lab, n * k * sizeof(int64_t))) ||
            (rows && (rc = stage_out(h, rows + q0 * k, h->sr_rows, n * k * sizeof(int64_t)))) ||
            (rc = stage_out(h, recons + q0 * k * d, h->rc_out, n * k * d * sizeof(float))))
            return rc;
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return check_status(h);
}
