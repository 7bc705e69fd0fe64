// Construction side: code books, encoding of vectors and groups, PQ training, exact neighbour tables, coarse k-means.
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

// residual against table[rows[i]] -> [OPQ] -> codes -> decode -> [OPQ back] -> + table row -> squared norm -> norm
// code, for m vectors in dx (clobbered).  Leaves the bytes in e_codes / e_ncodes.  The table is the centroid
// table (add_batch) or a batch's sub-centroid table (add_group).
int encode_rows(ivfhnsw_gpu *h, size_t m, float *dx, const float *table, const uint32_t *rows)
{
    const size_t d = h->e_d, M = h->e_M;
    float *res = h->e_res.as<float>(), *tmp = h->e_tmp.as<float>();
    HIP_TRY(launch_madd_rows(h->stream, dx, -1.f, table, rows, res, m, (int)d));
    const float *enc_in = res;
    if (h->e_opq) {
        HIP_TRY(launch_opq(h->stream, h->e_at.as<float>(), res, tmp, (int)m, (int)d));
        enc_in = tmp;
    }
    HIP_TRY(launch_pq_encode(h->stream, enc_in, h->e_pqc.as<float>(), h->e_codes.as<uint8_t>(), m, (int)d, (int)M));
    float *dec = h->e_opq ? res : tmp; // the buffer the encoder did not read
    HIP_TRY(launch_pq_decode(h->stream, h->e_codes.as<uint8_t>(), h->e_pqc.as<float>(), dec, m, (int)d, (int)M));
    float *back = dec;
    if (h->e_opq) {
        HIP_TRY(launch_opq(h->stream, h->e_a.as<float>(), dec, tmp, (int)m, (int)d));
        back = tmp;
    }
    HIP_TRY(launch_madd_rows(h->stream, back, 1.f, table, rows, dx, m, (int)d)); // x is spent: reuse
    HIP_TRY(launch_norm_codes(h->stream, dx, h->e_ntab.as<float>(), h->e_ncodes.as<uint8_t>(), nullptr, m, (int)d));
    return IVFHNSW_OK;
}

// centroid_idx and offsets are host arrays; dev: x and the out_* arrays are device pointers.  stage (add_groups): every
// chunk's list ids, sub-group ids, codes and norm codes also go to the append staging (ap_idx, gp_sub, ap_codes, ap_ncodes)
// and the groups' neighbour rows and alphas to ga_nn / ga_alpha, all sized by the caller.
int encode_groups_impl(ivfhnsw_gpu *h, size_t ngroups, size_t nsubc, const uint32_t *centroid_idx,
                              const uint64_t *offsets, const float *x, size_t efSearch, uint32_t *out_nn_centroid_idxs,
                              float *out_alphas, uint32_t *out_subcentroid_idxs, uint8_t *out_codes,
                              uint8_t *out_norm_codes, bool dev, bool stage)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_codebooks || !h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "encode_groups needs upload_codebooks and upload_quantizer");
    if ((size_t)h->gr.d != h->e_d)
        return fail(IVFHNSW_ERR_STATE, "code books are for d = %zu, the quantizer holds d = %d", h->e_d, h->gr.d);
    if (ngroups == 0)
        return IVFHNSW_OK;
    if (!centroid_idx || !offsets || !out_nn_centroid_idxs || !out_alphas)
        return fail(IVFHNSW_ERR_INVALID, "null buffer");
    const size_t d = h->e_d, M = h->e_M, k = nsubc + 1;
    if (nsubc == 0 || nsubc > 4096 || efSearch < k || k > h->gr.n)
        return fail(IVFHNSW_ERR_INVALID, "nsubc %zu: need 1 <= nsubc, nsubc + 1 <= efSearch (%zu) and <= %u centroids",
                    nsubc, efSearch, h->gr.n);
    if (group_points_lds_bytes((int)nsubc, (int)d) > 160 * 1024)
        return fail(IVFHNSW_ERR_INVALID, "nsubc %zu x d %zu does not fit the 160 KB of LDS of one workgroup", nsubc, d);
    if (offsets[0] != 0)
        return fail(IVFHNSW_ERR_INVALID, "offsets[0] must be 0");
    const uint64_t n_total = offsets[ngroups];
    for (size_t g = 0; g < ngroups; g++) {
        if (offsets[g + 1] < offsets[g])
            return fail(IVFHNSW_ERR_INVALID, "offsets not monotone at group %zu", g);
        if (centroid_idx[g] >= h->gr.n)
            return fail(IVFHNSW_ERR_INVALID, "centroid_idx[%zu] = %u out of range", g, centroid_idx[g]);
    }
    if (n_total && (!x || !out_subcentroid_idxs || !out_codes || (!out_norm_codes && !stage)))
        return fail(IVFHNSW_ERR_INVALID, "null buffer");
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    // chunks of whole groups: at most 2^18 points (one oversized group goes alone) and 4096 groups
    const size_t kMaxPoints = (size_t)1 << 18, kMaxGroups = 4096;
    std::vector<uint32_t> ids, nn;
    std::vector<float> dists, cvn;
    std::vector<unsigned long long> off;
    for (size_t g0 = 0; g0 < ngroups;) {
        size_t g1 = g0 + 1;
        while (g1 < ngroups && g1 - g0 < kMaxGroups && offsets[g1 + 1] - offsets[g0] <= kMaxPoints)
            g1++;
        const size_t G = g1 - g0, p0 = offsets[g0], m = offsets[g1] - p0;
        // neighbour centroids: searchKnn(centroid, nsubc + 1) for every group of the chunk (Grouping.cpp:47-62)
        if ((rc = h->cg_q.ensure(G * d * sizeof(float))) || (rc = h->cg_cidx.ensure(G * sizeof(uint32_t))) ||
            (rc = h->cg_ids.ensure(G * k * sizeof(uint32_t))) || (rc = h->cg_dists.ensure(G * k * sizeof(float))) ||
            (rc = h->gc_nn.ensure(G * nsubc * sizeof(uint32_t))) || (rc = h->cg_cvn.ensure(G * nsubc * sizeof(float))) ||
            (rc = h->cg_tab.ensure(G * nsubc * d * sizeof(float))) || (rc = h->cg_tab2.ensure(G * nsubc * d * sizeof(float))) ||
            (rc = h->cg_off.ensure((G + 1) * sizeof(unsigned long long))) || (rc = h->cg_alpha2.ensure(G * sizeof(float))))
            return rc;
        HIP_TRY(hipMemcpyAsync(h->cg_cidx.p, centroid_idx + g0, G * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemsetAsync(h->cg_q.p, 0, G * d * sizeof(float), h->stream));
        HIP_TRY(launch_madd_rows(h->stream, h->cg_q.as<float>(), 1.f, h->gr.vectors, h->cg_cidx.as<uint32_t>(),
                                 h->cg_q.as<float>(), G, (int)d)); // 0 + 1 * row: the centroid rows as queries
        if ((rc = ivfhnsw_gpu_coarse_dev(h, G, h->cg_q.as<float>(), k, efSearch, h->cg_ids.as<uint32_t>(),
                                         h->cg_dists.as<float>())))
            return rc;
        ids.resize(G * k);
        dists.resize(G * k);
        HIP_TRY(hipMemcpyAsync(ids.data(), h->cg_ids.p, G * k * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(dists.data(), h->cg_dists.p, G * k * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if ((rc = check_status(h)))
            return rc;
        nn.resize(G * nsubc);
        cvn.resize(G * nsubc);
        for (size_t g = 0; g < G; g++)
            for (size_t s = 0; s < nsubc; s++) { // the nearest one (the centroid itself) is dropped
                if (ids[g * k + s + 1] == 0xffffffffu)
                    return fail(IVFHNSW_ERR_INVALID, "group %zu: the walk found fewer than nsubc + 1 = %zu centroids "
                                                     "(the reference leaves zero entries behind here)", g0 + g, k);
                nn[g * nsubc + s] = ids[g * k + s + 1];
                cvn[g * nsubc + s] = dists[g * k + s + 1];
            }
        if (dev)
            HIP_TRY(hipMemcpy(out_nn_centroid_idxs + g0 * nsubc, nn.data(), G * nsubc * sizeof(uint32_t), hipMemcpyHostToDevice));
        else
            std::memcpy(out_nn_centroid_idxs + g0 * nsubc, nn.data(), G * nsubc * sizeof(uint32_t));
        if (stage)
            HIP_TRY(hipMemcpy(h->ga_nn.as<uint32_t>() + g0 * nsubc, nn.data(), G * nsubc * sizeof(uint32_t),
                              hipMemcpyHostToDevice));
        if (m == 0) { // only empty groups: alpha stays what the caller has (Grouping.cpp:63-64)
            g0 = g1;
            continue;
        }
        off.resize(G + 1);
        for (size_t g = 0; g <= G; g++)
            off[g] = offsets[g0 + g] - p0;
        if ((rc = h->e_x.ensure(m * d * sizeof(float))) || (rc = h->e_res.ensure(m * d * sizeof(float))) ||
            (rc = h->e_tmp.ensure(m * d * sizeof(float))) || (rc = h->e_idx.ensure(m * sizeof(uint32_t))) ||
            (rc = h->e_dist.ensure(2 * m * sizeof(float))) || (rc = h->e_codes.ensure(m * M)) ||
            (rc = h->e_ncodes.ensure(m)) || (rc = h->cg_sub.ensure(m * sizeof(uint32_t))))
            return rc;
        float *dx = h->e_x.as<float>();
        HIP_TRY(hipMemcpyAsync(dx, x + p0 * d, m * d * sizeof(float), in, h->stream));
        HIP_TRY(hipMemcpyAsync(h->gc_nn.p, nn.data(), G * nsubc * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->cg_cvn.p, cvn.data(), G * nsubc * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->cg_off.p, off.data(), (G + 1) * sizeof(unsigned long long), hipMemcpyHostToDevice, h->stream));
        const uint32_t *cidx = h->cg_cidx.as<uint32_t>();
        const unsigned long long *doff = h->cg_off.as<unsigned long long>();
        float *cv = h->cg_tab.as<float>(), *sub = h->cg_tab2.as<float>(), *num = h->e_dist.as<float>(), *den = num + m;
        HIP_TRY(launch_group_table(h->stream, 0, h->gr.vectors, cidx, (const uint32_t *)h->gc_nn.p, nullptr, nullptr, cv, G,
                                   (int)nsubc, (int)d));
        HIP_TRY(launch_group_points(h->stream, 0, h->gr.vectors, cidx, cv, h->cg_cvn.as<float>(), doff, dx, num, den,
                                    nullptr, G, (int)nsubc, (int)d));
        HIP_TRY(launch_group_alpha(h->stream, doff, num, den, h->cg_alpha2.as<float>(), G));
        HIP_TRY(launch_group_table(h->stream, 1, h->gr.vectors, cidx, nullptr, h->cg_alpha2.as<float>(), cv, sub, G,
                                   (int)nsubc, (int)d));
        HIP_TRY(launch_group_points(h->stream, 1, h->gr.vectors, cidx, sub, nullptr, doff, dx, nullptr, nullptr,
                                    h->cg_sub.as<uint32_t>(), G, (int)nsubc, (int)d));
        HIP_TRY(launch_group_rows(h->stream, doff, h->cg_sub.as<uint32_t>(), h->e_idx.as<uint32_t>(), G, (int)nsubc));
        if ((rc = encode_rows(h, m, dx, sub, h->e_idx.as<uint32_t>())))
            return rc;
        // alphas: only groups with points are written (an empty group keeps the caller's value)
        std::vector<float> al(G);
        HIP_TRY(hipMemcpyAsync(al.data(), h->cg_alpha2.p, G * sizeof(float), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(out_subcentroid_idxs + p0, h->cg_sub.p, m * sizeof(uint32_t), out, h->stream));
        HIP_TRY(hipMemcpyAsync(out_codes + p0 * M, h->e_codes.p, m * M, out, h->stream));
        if (out_norm_codes)
            HIP_TRY(hipMemcpyAsync(out_norm_codes + p0, h->e_ncodes.p, m, out, h->stream));
        if (stage) { // the codes stay in HBM on their way into the lists
            HIP_TRY(launch_groups_point_lists(h->stream, doff, cidx, G, h->ap_idx.as<uint32_t>() + p0));
            HIP_TRY(hipMemcpyAsync(h->gp_sub.as<uint32_t>() + p0, h->cg_sub.p, m * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->ap_codes.as<uint8_t>() + p0 * M, h->e_codes.p, m * M, hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->ap_ncodes.as<uint8_t>() + p0, h->e_ncodes.p, m, hipMemcpyDeviceToDevice, h->stream));
            HIP_TRY(hipMemcpyAsync(h->ga_alpha.as<float>() + g0, h->cg_alpha2.p, G * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        }
        HIP_TRY(hipStreamSynchronize(h->stream));
        std::vector<float> cur(G); // an empty group keeps the caller's alpha
        if (dev)
            HIP_TRY(hipMemcpy(cur.data(), out_alphas + g0, G * sizeof(float), hipMemcpyDeviceToHost));
        float *dst = dev ? cur.data() : out_alphas + g0;
        for (size_t g = 0; g < G; g++)
            if (off[g + 1] > off[g])
                dst[g] = al[g];
        if (dev)
            HIP_TRY(hipMemcpy(out_alphas + g0, cur.data(), G * sizeof(float), hipMemcpyHostToDevice));
        g0 = g1;
    }
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_upload_codebooks(ivfhnsw_gpu *h, size_t d, size_t code_size, const float *pq_centroids,
                                 const float *norm_table, const float *opq_A)
try {
    int rc = table_change_guard(h, kUploads, "upload_codebooks", false);
    if (rc)
        return rc;
    if (d == 0 || code_size == 0 || d % code_size || d / code_size > 64 || !pq_centroids || !norm_table)
        return fail(IVFHNSW_ERR_INVALID, "bad code books (d %zu, code_size %zu)", d, code_size);
    h->has_codebooks = false;
    if ((rc = upload(h->e_pqc, pq_centroids, 256 * d * sizeof(float))))
        return rc;
    if ((rc = upload(h->e_ntab, norm_table, 256 * sizeof(float))))
        return rc;
    h->e_opq = opq_A != nullptr;
    if (opq_A) {
        // both orientations: apply reads A transposed, transform_transpose reads it as it is (launch_opq takes
        // the matrix of y = B x stored as B^T)
        std::vector<float> at(d * d);
        for (size_t i = 0; i < d; i++)
            for (size_t k = 0; k < d; k++)
                at[k * d + i] = opq_A[i * d + k];
        if ((rc = upload(h->e_at, at.data(), d * d * sizeof(float))))
            return rc;
        if ((rc = upload(h->e_a, opq_A, d * d * sizeof(float))))
            return rc;
    }
    h->e_d = d;
    h->e_M = code_size;
    h->has_codebooks = true;
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "ivfhnsw_gpu_upload_codebooks: host allocation failed");
}

int ivfhnsw_gpu_encode(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *precomputed_idx, size_t efSearch,
                       uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_codebooks || !h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "encode needs upload_codebooks and upload_quantizer");
    if ((size_t)h->gr.d != h->e_d)
        return fail(IVFHNSW_ERR_STATE, "code books are for d = %zu, the quantizer holds d = %d", h->e_d, h->gr.d);
    if (n == 0)
        return IVFHNSW_OK;
    if (!x || !out_codes || !out_norm_codes)
        return fail(IVFHNSW_ERR_INVALID, "null buffer");
    if (!precomputed_idx && efSearch == 0)
        return fail(IVFHNSW_ERR_INVALID, "efSearch 0 (assign runs searchKnn(x, 1))");
    const size_t d = h->e_d, M = h->e_M;
    const size_t kChunk = (size_t)1 << 18; // 128 MB of vectors at d = 128 per buffer
    for (size_t i0 = 0; i0 < n; i0 += kChunk) {
        const size_t m = std::min(kChunk, n - i0);
        if ((rc = h->e_x.ensure(m * d * sizeof(float))) || (rc = h->e_res.ensure(m * d * sizeof(float))) ||
            (rc = h->e_tmp.ensure(m * d * sizeof(float))) || (rc = h->e_idx.ensure(m * sizeof(uint32_t))) ||
            (rc = h->e_dist.ensure(m * sizeof(float))) || (rc = h->e_codes.ensure(m * M)) ||
            (rc = h->e_ncodes.ensure(m)))
            return rc;
        float *dx = h->e_x.as<float>();
        uint32_t *idx = h->e_idx.as<uint32_t>();
        HIP_TRY(hipMemcpyAsync(dx, x + i0 * d, m * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
        if (precomputed_idx) {
            for (size_t i = 0; i < m; i++)
                if (precomputed_idx[i0 + i] >= h->gr.n)
                    return fail(IVFHNSW_ERR_INVALID, "precomputed_idx[%zu] = %u out of range", i0 + i,
                                precomputed_idx[i0 + i]);
            HIP_TRY(hipMemcpyAsync(idx, precomputed_idx + i0, m * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        } else if ((rc = ivfhnsw_gpu_coarse_dev(h, m, dx, 1, efSearch, idx, h->e_dist.as<float>()))) {
            return rc;
        }
        if ((rc = encode_rows(h, m, dx, h->gr.vectors, idx)))
            return rc;
        HIP_TRY(hipMemcpyAsync(out_codes + i0 * M, h->e_codes.p, m * M, hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(out_norm_codes + i0, h->e_ncodes.p, m, hipMemcpyDeviceToHost, h->stream));
        if (out_idx)
            HIP_TRY(hipMemcpyAsync(out_idx + i0, idx, m * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if ((rc = check_status(h)))
            return rc;
    }
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_encode_groups(ivfhnsw_gpu *h, size_t ngroups, size_t nsubc, const uint32_t *centroid_idx,
                              const uint64_t *offsets, const float *x, size_t efSearch, uint32_t *out_nn_centroid_idxs,
                              float *out_alphas, uint32_t *out_subcentroid_idxs, uint8_t *out_codes,
                              uint8_t *out_norm_codes)
try {
    return encode_groups_impl(h, ngroups, nsubc, centroid_idx, offsets, x, efSearch, out_nn_centroid_idxs, out_alphas,
                              out_subcentroid_idxs, out_codes, out_norm_codes, false, false);
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "ivfhnsw_gpu_encode_groups: host allocation failed");
}

int ivfhnsw_gpu_pq_train(ivfhnsw_gpu *h, size_t n, size_t d, size_t M, const float *x, size_t niter, float *centroids,
                         uint8_t *out_assign)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (n == 0 || d == 0 || M == 0 || d % M || d / M > 64 || !x || !centroids)
        return fail(IVFHNSW_ERR_INVALID, "bad training arguments (n %zu, d %zu, M %zu)", n, d, M);
    if ((rc = h->t_x.ensure(n * d * sizeof(float))) || (rc = h->t_cb.ensure(256 * d * sizeof(float))) ||
        (rc = h->t_assign.ensure(n * M)))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->t_x.p, x, n * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->t_cb.p, centroids, 256 * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    for (size_t it = 0; it < niter; it++) {
        // assignment = pq->compute_codes with the current code book; update = means in point order
        HIP_TRY(launch_pq_encode(h->stream, h->t_x.as<float>(), h->t_cb.as<float>(), h->t_assign.as<uint8_t>(), n, (int)d,
                                 (int)M));
        HIP_TRY(launch_lloyd_update(h->stream, h->t_x.as<float>(), h->t_assign.as<uint8_t>(), h->t_cb.as<float>(), n,
                                    (int)d, (int)M));
    }
    HIP_TRY(hipMemcpyAsync(centroids, h->t_cb.p, 256 * d * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (out_assign && niter)
        HIP_TRY(hipMemcpyAsync(out_assign, h->t_assign.p, n * M, hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_xty(ivfhnsw_gpu *h, size_t n, size_t d, const float *X, const float *Y, float *C)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (n == 0 || d == 0 || d > 4096 || !X || !Y || !C)
        return fail(IVFHNSW_ERR_INVALID, "bad xty arguments (n %zu, d %zu)", n, d);
    const size_t nchunks = (n + kXtyChunk - 1) / kXtyChunk;
    if (nchunks > 65535)
        return fail(IVFHNSW_ERR_INVALID, "xty: more than %d points", 65535 * kXtyChunk);
    if ((rc = h->t_x.ensure(n * d * sizeof(float))) || (rc = h->t_y.ensure(n * d * sizeof(float))) ||
        (rc = h->t_part.ensure(nchunks * d * d * sizeof(float))) || (rc = h->t_c.ensure(d * d * sizeof(float))))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->t_x.p, X, n * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->t_y.p, Y, n * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(launch_xty(h->stream, h->t_x.as<float>(), h->t_y.as<float>(), h->t_part.as<float>(), h->t_c.as<float>(), n,
                       (int)d));
    HIP_TRY(hipMemcpyAsync(C, h->t_c.p, d * d * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_knn_dev(ivfhnsw_gpu *h, size_t nq, size_t nx, size_t d, const float *d_queries, const float *d_base,
                        size_t k, int mode, uint32_t *d_out_ids, float *d_out_dists)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (d < 4 || d > 128 || (d & 3))
        return fail(IVFHNSW_ERR_INVALID, "knn: d %zu must be a multiple of 4, at most 128", d);
    if (k == 0 || k > 80)
        return fail(IVFHNSW_ERR_INVALID, "knn: k %zu outside 1..80", k);
    if (nq > 0x7fffffffull || nx > 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "knn: too many rows");
    if (mode < IVFHNSW_KNN_ALL || mode > IVFHNSW_KNN_EARLIER)
        return fail(IVFHNSW_ERR_INVALID, "knn: unknown mode %d", mode);
    if (nq == 0)
        return IVFHNSW_OK;
    if (!d_queries || !d_base || !d_out_ids)
        return fail(IVFHNSW_ERR_INVALID, "knn: null buffer");
    // (the triangular table is one sweep per row block: its column range depends on the block)
    const int nsplit = mode == IVFHNSW_KNN_EARLIER ? 1 : knn_splits_for(nq, nx ? nx : 1);
    if ((rc = h->k_qn.ensure(nq * sizeof(float))) || (rc = h->k_xn.ensure((nx ? nx : 1) * sizeof(float))) ||
        (rc = h->k_part.ensure((size_t)nsplit * nq * k * sizeof(uint64_t))))
        return rc;
    float *dd = d_out_dists;
    if (!dd) {
        if ((rc = h->k_dists.ensure(nq * k * sizeof(float))))
            return rc;
        dd = h->k_dists.as<float>();
    }
    HIP_TRY(launch_knn_norms(h->stream, d_queries, h->k_qn.as<float>(), nq, (int)d));
    HIP_TRY(launch_knn_norms(h->stream, d_base, h->k_xn.as<float>(), nx, (int)d));
    HIP_TRY(launch_knn(h->stream, d_queries, d_base, h->k_qn.as<float>(), h->k_xn.as<float>(), nq, nx, (int)d, (int)k,
                       mode, nsplit, h->k_part.as<unsigned long long>(), d_out_ids, dd));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_knn(ivfhnsw_gpu *h, size_t nq, size_t nx, size_t d, const float *queries, const float *base, size_t k,
                    int mode, uint32_t *out_ids, float *out_dists)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!base || !out_ids)
        return fail(IVFHNSW_ERR_INVALID, "knn: null buffer");
    const bool self = queries == nullptr;
    if (self)
        nq = nx;
    if (nq == 0)
        return IVFHNSW_OK;
    if ((rc = upload(h->k_x, base, nx * d * sizeof(float))))
        return rc;
    if (!self && (rc = upload(h->k_q, queries, nq * d * sizeof(float))))
        return rc;
    if ((rc = h->k_ids.ensure(nq * k * sizeof(uint32_t))) || (rc = h->k_dists.ensure(nq * k * sizeof(float))))
        return rc;
    // (k_dists doubles as the output buffer here: knn_dev is handed it explicitly, so it does not allocate its own)
    if ((rc = ivfhnsw_gpu_knn_dev(h, nq, nx, d, self ? h->k_x.as<float>() : h->k_q.as<float>(), h->k_x.as<float>(), k,
                                  mode, h->k_ids.as<uint32_t>(), h->k_dists.as<float>())))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out_ids, h->k_ids.p, nq * k * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (out_dists)
        HIP_TRY(hipMemcpy(out_dists, h->k_dists.p, nq * k * sizeof(float), hipMemcpyDeviceToHost));
    return IVFHNSW_OK;
}

namespace {

// what both forms of build_graph refuse, before either touches a buffer (vectors / counts / links: host or device)
int build_graph_check(ivfhnsw_gpu *h, size_t n, size_t d, const void *vectors, size_t M, size_t maxM, size_t ncand,
                      const void *counts, const void *links)
{
    if (!h || !vectors || !counts || !links)
        return fail(IVFHNSW_ERR_INVALID, "build_graph: null argument");
    if (M < 1 || M > maxM || maxM > 64 || ncand < M || ncand > 80 || n >= 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "build_graph: need 1 <= M <= maxM <= 64, M <= ncand <= 80, n < 2^32");
    if (d % 16 != 0)
        return fail(IVFHNSW_ERR_INVALID, "build_graph: d must be a multiple of 16 (the reference's distance "
                                         "ignores the dims beyond one, hnswalg.cpp:330; so does upload_quantizer)");
    if (n > 1 && (d < 16 || d > 128))
        return fail(IVFHNSW_ERR_INVALID, "knn: d %zu must be a multiple of 4, at most 128", d);
    if (n > 0x7fffffffull)
        return fail(IVFHNSW_ERR_INVALID, "knn: too many rows");
    if (n * M > 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "build_graph: n * M must stay below 2^32 (the reverse lists are indexed by 32 bits)");
    return IVFHNSW_OK;
}

int kmeans_check(ivfhnsw_gpu *h, size_t n, size_t d, size_t nc, const void *x, const void *c)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (d < 4 || d > 128 || (d & 3))
        return fail(IVFHNSW_ERR_INVALID, "kmeans: d %zu must be a multiple of 4, at most 128", d);
    if (nc < 1 || nc > n || n > 0x7fffffffull)
        return fail(IVFHNSW_ERR_INVALID, "kmeans: need 1 <= nc <= n < 2^31 (n %zu, nc %zu)", n, nc);
    if (!x || !c)
        return fail(IVFHNSW_ERR_INVALID, "kmeans: null buffer");
    return IVFHNSW_OK;
}

// faiss's split_clusters with the random choice replaced: every empty cluster ci, ascending, takes the cluster cj with
// the largest CURRENT count (ties to the lower id); cnt[ci] = cnt[cj] / 2, cnt[cj] -= cnt[ci].  n >= nc keeps a count
// >= 2 in the heap while a cluster is empty, so ci never stays empty.  Heap entries are (count, ~id); an entry whose
// count is no longer the cluster's is stale (a split only lowers cj's count) and is dropped when it surfaces.
void kmeans_pick_splits(std::vector<uint32_t> &cnt, std::vector<uint32_t> &pairs)
{
    pairs.clear();
    std::vector<std::pair<uint32_t, uint32_t>> heap;
    for (size_t c = 0; c < cnt.size(); c++)
        if (cnt[c])
            heap.emplace_back(cnt[c], ~(uint32_t)c);
    if (heap.size() == cnt.size())
        return;
    std::make_heap(heap.begin(), heap.end());
    for (size_t ci = 0; ci < cnt.size(); ci++) {
        if (cnt[ci])
            continue;
        uint32_t cj;
        for (;;) {
            std::pop_heap(heap.begin(), heap.end());
            const auto top = heap.back();
            heap.pop_back();
            cj = ~top.second;
            if (top.first == cnt[cj])
                break;
        }
        cnt[ci] = cnt[cj] / 2;
        cnt[cj] -= cnt[ci];
        pairs.push_back((uint32_t)ci);
        pairs.push_back(cj);
        heap.emplace_back(cnt[cj], ~cj);
        std::push_heap(heap.begin(), heap.end());
        heap.emplace_back(cnt[ci], ~(uint32_t)ci);
        std::push_heap(heap.begin(), heap.end());
    }
}

// niter Lloyd iterations on device buffers: assign (knn k = 1), objective, counts, stable member lists,
// means, splits.  One synchronisation per iteration: the counts and the objective's partial sums come to the host.
int kmeans_run(ivfhnsw_gpu *h, size_t n, size_t d, size_t nc, const float *d_x, size_t niter, float *d_c,
               uint32_t *d_out_assign, double *out_obj) try
{
    const size_t nblocks = (n + kKmeansTile - 1) / kKmeansTile;
    int rc;
    if ((rc = h->km_assign.ensure(n * sizeof(uint32_t))) || (rc = h->km_dist.ensure(n * sizeof(float))) ||
        (rc = h->km_ids.ensure(n * sizeof(uint32_t))) || (rc = h->km_ids2.ensure(n * sizeof(uint32_t))) ||
        (rc = h->km_cnt.ensure(nc * sizeof(uint32_t))) || (rc = h->km_start.ensure(nc * sizeof(uint32_t))) ||
        (rc = h->km_hist.ensure(256 * nblocks * sizeof(uint32_t))) || (rc = h->km_part.ensure(nblocks * sizeof(double))) ||
        (rc = h->km_status.ensure(sizeof(uint32_t))) || (rc = h->km_pairs.ensure(2 * nc * sizeof(uint32_t))))
        return rc;
    int key_bits = 0;
    while (key_bits < 32 && ((nc - 1) >> key_bits))
        key_bits++;
    uint32_t *assign = h->km_assign.as<uint32_t>(), *cnt = h->km_cnt.as<uint32_t>();
    std::vector<uint32_t> hcnt(nc), pairs;
    std::vector<double> hpart(nblocks);
    uint32_t status = 0;
    for (size_t it = 0; it < niter; it++) {
        if ((rc = ivfhnsw_gpu_knn_dev(h, n, nc, d, d_x, d_c, 1, IVFHNSW_KNN_ALL, assign, h->km_dist.as<float>())))
            return rc;
        HIP_TRY(hipMemsetAsync(cnt, 0, nc * sizeof(uint32_t), h->stream));
        HIP_TRY(hipMemsetAsync(h->km_status.p, 0, sizeof(uint32_t), h->stream));
        HIP_TRY(launch_kmeans_count(h->stream, assign, h->km_dist.as<float>(), n, (uint32_t)nc, cnt,
                                    h->km_part.as<double>(), h->km_status.as<uint32_t>()));
        HIP_TRY(launch_scan_u32(h->stream, cnt, h->km_start.as<uint32_t>(), nc));
        uint32_t *members = nullptr;
        HIP_TRY(launch_sort_by_key(h->stream, assign, n, key_bits, h->km_ids.as<uint32_t>(), h->km_ids2.as<uint32_t>(),
                                   h->km_hist.as<uint32_t>(), &members));
        HIP_TRY(launch_kmeans_means(h->stream, d_x, n, members, h->km_start.as<uint32_t>(), cnt, d_c, nc, (int)d));
        HIP_TRY(hipMemcpyAsync(hcnt.data(), cnt, nc * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(hpart.data(), h->km_part.p, nblocks * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(&status, h->km_status.p, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if (status)
            return fail(IVFHNSW_ERR_STATE, "kmeans: a point has no finite distance to any centroid (NaN or inf input)");
        if (out_obj) {
            double obj = 0.0;
            for (double p : hpart)
                obj += p;
            out_obj[it] = obj;
        }
        kmeans_pick_splits(hcnt, pairs);
        if (!pairs.empty()) {
            // pageable source: the copy has completed when the next iteration's synchronisation returns, before `pairs`
            // is rewritten
            HIP_TRY(hipMemcpyAsync(h->km_pairs.p, pairs.data(), pairs.size() * sizeof(uint32_t), hipMemcpyHostToDevice,
                                   h->stream));
            HIP_TRY(launch_kmeans_split(h->stream, d_c, h->km_pairs.as<uint32_t>(), pairs.size() / 2, (int)d));
        }
    }
    if (d_out_assign)
        HIP_TRY(hipMemcpyAsync(d_out_assign, assign, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "kmeans: host allocation failed");
}

} // namespace

int ivfhnsw_gpu_kmeans_dev(ivfhnsw_gpu *h, size_t n, size_t d, size_t nc, const float *d_x, size_t niter, float *d_centroids,
                           uint32_t *d_out_assign, double *out_obj)
{
    int rc = kmeans_check(h, n, d, nc, d_x, d_centroids);
    if (rc)
        return rc;
    if (((uintptr_t)d_x | (uintptr_t)d_centroids) & 15)
        return fail(IVFHNSW_ERR_INVALID, "kmeans_dev: x and centroids must be 16-byte aligned");
    if (niter == 0)
        return IVFHNSW_OK;
    return kmeans_run(h, n, d, nc, d_x, niter, d_centroids, d_out_assign, out_obj);
}

int ivfhnsw_gpu_kmeans(ivfhnsw_gpu *h, size_t n, size_t d, size_t nc, const float *x, size_t niter, float *centroids,
                       uint32_t *out_assign, double *out_obj)
{
    int rc = kmeans_check(h, n, d, nc, x, centroids);
    if (rc)
        return rc;
    if (niter == 0)
        return IVFHNSW_OK;
    if ((rc = h->km_x.ensure(n * d * sizeof(float))) || (rc = h->km_c.ensure(nc * d * sizeof(float))))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->km_x.p, x, n * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->km_c.p, centroids, nc * d * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if ((rc = kmeans_run(h, n, d, nc, h->km_x.as<float>(), niter, h->km_c.as<float>(), nullptr, out_obj)))
        return rc;
    HIP_TRY(hipMemcpy(centroids, h->km_c.p, nc * d * sizeof(float), hipMemcpyDeviceToHost));
    if (out_assign)
        HIP_TRY(hipMemcpy(out_assign, h->km_assign.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_build_graph_dev(ivfhnsw_gpu *h, size_t n, size_t d, const float *d_vectors, size_t M, size_t maxM,
                                size_t ncand, uint8_t *d_out_counts, uint32_t *d_out_links)
{
    int rc = build_graph_check(h, n, d, d_vectors, M, maxM, ncand, d_out_counts, d_out_links);
    if (rc)
        return rc;
    if (((uintptr_t)d_vectors & 15) || ((uintptr_t)d_out_links & 3))
        return fail(IVFHNSW_ERR_INVALID, "build_graph_dev: vectors must be 16-byte aligned, links 4-byte aligned");
    if ((rc = bind(h)))
        return rc;
    if (n == 0)
        return IVFHNSW_OK;
    HIP_TRY(hipMemsetAsync(d_out_counts, 0, n, h->stream));
    HIP_TRY(hipMemsetAsync(d_out_links, 0, n * maxM * sizeof(uint32_t), h->stream));
    if (n == 1)
        return IVFHNSW_OK;
    const size_t nslots = n * M, nblocks = (nslots + kKmeansTile - 1) / kKmeansTile;
    if ((rc = h->gb_table.ensure(n * ncand * sizeof(uint32_t))) || (rc = h->gb_fwd.ensure(nslots * sizeof(uint32_t))) ||
        (rc = h->gb_fcnt.ensure(n)) || (rc = h->gb_deg.ensure((n + 1) * sizeof(uint32_t))) ||
        (rc = h->gb_roff.ensure((n + 1) * sizeof(uint32_t))) || (rc = h->gb_ids.ensure(nslots * sizeof(uint32_t))) ||
        (rc = h->gb_ids2.ensure(nslots * sizeof(uint32_t))) || (rc = h->gb_hist.ensure(256 * nblocks * sizeof(uint32_t))) ||
        (rc = h->gb_stat.ensure(sizeof(uint32_t))))
        return rc;
    uint32_t *table = h->gb_table.as<uint32_t>(), *fwd = h->gb_fwd.as<uint32_t>(), *deg = h->gb_deg.as<uint32_t>();
    // the exact candidates: row c against rows 0..c-1
    if ((rc = ivfhnsw_gpu_knn_dev(h, n, n, d, d_vectors, d_vectors, ncand, IVFHNSW_KNN_EARLIER, table, nullptr)))
        return rc;
    // A. forward links, and how many later nodes chose each node
    HIP_TRY(hipMemsetAsync(deg, 0, (n + 1) * sizeof(uint32_t), h->stream));
    HIP_TRY(hipMemsetAsync(h->gb_stat.p, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(launch_graph_forward(h->stream, d_vectors, table, n, (int)d, (int)M, (int)ncand, fwd, h->gb_fcnt.as<uint8_t>(), deg));
    // B. reverse lists: the link slots c * M + i sorted stably by the node they name (an empty slot names n, behind every
    // node), so that node t's run lists the nodes that chose it ascending -- the order the serial loop meets them in
    HIP_TRY(launch_scan_u32(h->stream, deg, h->gb_roff.as<uint32_t>(), n + 1));
    int key_bits = 1;
    while (key_bits < 32 && (n >> key_bits))
        key_bits++;
    uint32_t *pairs = nullptr;
    HIP_TRY(launch_sort_by_key(h->stream, fwd, nslots, key_bits, h->gb_ids.as<uint32_t>(), h->gb_ids2.as<uint32_t>(),
                               h->gb_hist.as<uint32_t>(), &pairs));
    // C. every node's own insertion, then the later nodes that chose it, in their order
    HIP_TRY(launch_graph_fold(h->stream, d_vectors, fwd, h->gb_fcnt.as<uint8_t>(), h->gb_roff.as<uint32_t>(), pairs, n, (int)d,
                              (int)M, (int)maxM, d_out_counts, d_out_links, h->gb_stat.as<uint32_t>()));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_build_graph(ivfhnsw_gpu *h, size_t n, size_t d, const float *vectors, size_t M, size_t maxM, size_t ncand,
                            uint8_t *out_counts, uint32_t *out_links)
{
    int rc = build_graph_check(h, n, d, vectors, M, maxM, ncand, out_counts, out_links);
    if (rc)
        return rc;
    if (n <= 1) {
        std::memset(out_counts, 0, n);
        std::memset(out_links, 0, n * maxM * sizeof(uint32_t));
        return IVFHNSW_OK;
    }
    if ((rc = bind(h)))
        return rc;
    if ((rc = upload(h->k_x, vectors, n * d * sizeof(float))) || (rc = h->gb_counts.ensure(n)) ||
        (rc = h->gb_links.ensure(n * maxM * sizeof(uint32_t))))
        return rc;
    if ((rc = ivfhnsw_gpu_build_graph_dev(h, n, d, h->k_x.as<float>(), M, maxM, ncand, h->gb_counts.as<uint8_t>(),
                                          h->gb_links.as<uint32_t>())))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(out_counts, h->gb_counts.p, n, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(out_links, h->gb_links.p, n * maxM * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_last_graph_longest_reverse(ivfhnsw_gpu *h, uint64_t *out)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!out)
        return fail(IVFHNSW_ERR_INVALID, "null argument");
    uint32_t v = 0;
    if (h->gb_stat.p) {
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(&v, h->gb_stat.p, sizeof(uint32_t), hipMemcpyDeviceToHost));
    }
    *out = v;
    return IVFHNSW_OK;
}
