// Uploads and downloads of the index tables: IVF lists, Grouping tables, the HNSW quantizer and its derived rows.
#include "capi_internal.h"
#include "walk_bound.h"
#include "walk_form.h"

namespace {

int check_desc(const ivfhnsw_ivf_desc *d, bool need_lists)
{
    if (!d)
        return fail(IVFHNSW_ERR_INVALID, "null descriptor");
    if (d->d == 0 || d->nc == 0 || d->code_size == 0)
        return fail(IVFHNSW_ERR_INVALID, "d, nc and code_size must be positive");
    if (d->code_size % 4)
        return fail(IVFHNSW_ERR_INVALID, "code_size %zu is not a multiple of 4 (IndexIVF_HNSW.cpp:805)", d->code_size);
    if (d->code_size * 1024 > kScanDynLdsMax)
        return fail(IVFHNSW_ERR_INVALID, "code_size %zu: the query's table (1 KB per code byte) must fit %zu KB of LDS",
                    d->code_size, kScanDynLdsMax / 1024);
    if (d->d % d->code_size)
        return fail(IVFHNSW_ERR_INVALID, "d %zu is not a multiple of code_size %zu", d->d, d->code_size);
    if (d->d / d->code_size > 64)
        return fail(IVFHNSW_ERR_INVALID, "sub-vector dimension %zu > 64 unsupported", d->d / d->code_size);
    if (d->nc >= 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "nc too large");
    if (!d->offsets || !d->centroid_norms || !d->pq_centroids || !d->norm_table)
        return fail(IVFHNSW_ERR_INVALID, "offsets, centroid_norms, pq_centroids and norm_table are required");
    if (need_lists && d->offsets[d->nc] != 0 && (!d->ids || !d->codes || !d->norm_codes))
        return fail(IVFHNSW_ERR_INVALID, "ids, codes and norm_codes are required");
    if (d->shard_world == 0 || d->shard_rank >= d->shard_world)
        return fail(IVFHNSW_ERR_INVALID, "bad shard %u of %u", d->shard_rank, d->shard_world);
    if (d->offsets[0] != 0)
        return fail(IVFHNSW_ERR_INVALID, "offsets[0] must be 0");
    for (size_t c = 0; c < d->nc; c++)
        if (d->offsets[c + 1] < d->offsets[c])
            return fail(IVFHNSW_ERR_INVALID, "offsets not monotone at list %zu", c);
    return IVFHNSW_OK;
}

// The descriptor's check and the tables shared by upload_ivf and upload_ivf_synthetic; fills h->t except
// codes/norm_codes/ids.  The handle holds no index until the caller has filled the lists.
int upload_tables(ivfhnsw_gpu *h, const ivfhnsw_ivf_desc *d, bool need_lists, uint64_t &n_local)
{
    int rc = check_desc(d, need_lists);
    if (rc)
        return rc;
    h->has_ivf = false;
    filter_drop(h); // a filter belongs to the lists it was marked over
    slots_drop(h);  // ... and so do the filter slots
    tags_drop(h);   // ... and the row tags
    values_drop(h); // ... and the row values
    range_drop(h);  // ... and range results to the lists they were found in
    std::vector<uint32_t> loff(d->nc, kNotOwned);
    n_local = 0;
    for (size_t c = 0; c < d->nc; c++) {
        const uint32_t owner = d->list_owner ? d->list_owner[c] : (uint32_t)(c % d->shard_world);
        if (owner >= d->shard_world)
            return fail(IVFHNSW_ERR_INVALID, "list_owner[%zu] = %u is not a rank of %u", c, owner, d->shard_world);
        if (owner != d->shard_rank)
            continue;
        if (n_local >= 0xffffffffull)
            return fail(IVFHNSW_ERR_INVALID, "2^32 - 1 or more codes on one shard");
        loff[c] = (uint32_t)n_local;
        n_local += d->offsets[c + 1] - d->offsets[c];
    }
    if (n_local >= 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "2^32 - 1 or more codes on one shard");
    if ((rc = upload(h->goff, d->offsets, (d->nc + 1) * sizeof(uint64_t))))
        return rc;
    if ((rc = upload(h->loff, loff.data(), d->nc * sizeof(uint32_t))))
        return rc;
    if ((rc = upload(h->cnorm, d->centroid_norms, d->nc * sizeof(float))))
        return rc;
    if ((rc = upload(h->pqc, d->pq_centroids, 256 * d->d * sizeof(float))))
        return rc;
    if ((rc = upload(h->ntab, d->norm_table, 256 * sizeof(float))))
        return rc;
    if (d->opq_A) {
        std::vector<float> at(d->d * d->d);
        for (size_t i = 0; i < d->d; i++)
            for (size_t k = 0; k < d->d; k++)
                at[k * d->d + i] = d->opq_A[i * d->d + k];
        if ((rc = upload(h->opq_at, at.data(), at.size() * sizeof(float))))
            return rc;
        if ((rc = upload(h->opq_a, d->opq_A, at.size() * sizeof(float)))) // as given: ORIGINAL-space reconstruction (capi_recon.cpp)
            return rc;
    } else {
        h->opq_at.release();
        h->opq_a.release();
    }
    IvfTables &t = h->t;
    t.d = (int)d->d;
    t.M = (int)d->code_size;
    t.dsub = (int)(d->d / d->code_size);
    t.nc = (uint32_t)d->nc;
    t.goff = h->goff.as<uint64_t>();
    t.loff = h->loff.as<uint32_t>();
    t.centroid_norms = h->cnorm.as<float>();
    t.pq_centroids = h->pqc.as<float>();
    t.norm_table = h->ntab.as<float>();
    t.opq_At = d->opq_A ? h->opq_at.as<float>() : nullptr;
    h->opq_A = d->opq_A ? h->opq_a.as<float>() : nullptr;
    t.shard_rank = d->shard_rank;
    t.shard_world = d->shard_world;
    return IVFHNSW_OK;
}

// The dedupe choice of a Grouping index (see grouping_dedupe below) over row accessors, so that a caller holding only the
// sampled rows can ask the same question.
// sizes_row(c) / nn_row(c): row c of the two tables (only the sampled groups' rows and their neighbours' are asked for)
template <class SizesRow, class NnRow>
int grouping_dedupe_rows(size_t nc, size_t nsubc, SizesRow sizes_row, NnRow nn_row)
{
    const size_t take = std::min<size_t>(15, nsubc), step = std::max<size_t>(1, nc / 512);
    double distinct = 0, total = 0;
    // distinct ids of a sample by the sample's number stamped on the id (ids of non-empty sub-groups are < nc, checked at
    // upload; any other id is counted by sort + unique): sorting every sample cost about 15 ms per call at nsubc 64, DESIGN.md 3.12
    std::vector<uint32_t> seen(nc, 0), odd;
    uint32_t stamp = 0;
    for (size_t c = 0; c < nc; c += step) {
        odd.clear();
        stamp++;
        auto add_list = [&](size_t cc) {
            const uint32_t *sz = sizes_row(cc), *nn = nn_row(cc);
            for (size_t j = 0; j < nsubc; j++) {
                if (!sz[j])
                    continue;
                total += 1.0;
                if (nn[j] >= nc) {
                    odd.push_back(nn[j]);
                } else if (seen[nn[j]] != stamp) {
                    seen[nn[j]] = stamp;
                    distinct += 1.0;
                }
            }
        };
        add_list(c);
        const uint32_t *nn_c = nn_row(c);
        for (size_t j = 0; j < take; j++)
            if (nn_c[j] < nc)
                add_list(nn_c[j]);
        std::sort(odd.begin(), odd.end());
        distinct += (double)(std::unique(odd.begin(), odd.end()) - odd.begin());
    }
    return (total > 0 && distinct / total < 0.55) ? 1 : 0;
}

} // namespace

namespace ivfhnsw_gpu_impl {

// the device buffers grouping_dedupe_dev can need, sized for its largest sample, so that it allocates nothing itself
int grouping_dedupe_reserve(ivfhnsw_gpu *h)
{
    const size_t nc = h->t.nc, nsubc = (size_t)h->g.nsubc;
    const size_t take = std::min<size_t>(15, nsubc), step = std::max<size_t>(1, nc / 512);
    const size_t rows = ((nc + step - 1) / step) * (1 + take);
    int rc;
    if ((rc = h->gp_rows.ensure(rows * sizeof(uint32_t))) || (rc = h->gp_gather.ensure(2 * rows * nsubc * sizeof(uint32_t))))
        return rc;
    return IVFHNSW_OK;
}

// grouping_dedupe on the tables in HBM: only the rows it samples (about 512 groups and 15 neighbours of each) come to
// the host, not the two [nc * nsubc] tables
int grouping_dedupe_dev(ivfhnsw_gpu *h, const uint32_t *d_sizes, const uint32_t *d_nn, int *dedupe)
{
    const size_t nc = h->t.nc, nsubc = (size_t)h->g.nsubc;
    const size_t take = std::min<size_t>(15, nsubc), step = std::max<size_t>(1, nc / 512);
    std::vector<uint32_t> want, szs, nns;
    std::unordered_map<uint32_t, size_t> at;
    int rc;
    auto fetch = [&](size_t first) -> int { // rows want[first ..] of both tables behind the ones already here
        const size_t m = want.size() - first;
        if (m == 0)
            return IVFHNSW_OK;
        if ((rc = h->gp_rows.ensure(m * sizeof(uint32_t))) || (rc = h->gp_gather.ensure(2 * m * nsubc * sizeof(uint32_t))))
            return rc;
        uint32_t *g = h->gp_gather.as<uint32_t>();
        HIP_TRY(hipMemcpyAsync(h->gp_rows.p, want.data() + first, m * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
        HIP_TRY(launch_gather_rows(h->stream, d_sizes, h->gp_rows.as<uint32_t>(), m, (uint32_t)nsubc, g));
        HIP_TRY(launch_gather_rows(h->stream, d_nn, h->gp_rows.as<uint32_t>(), m, (uint32_t)nsubc, g + m * nsubc));
        szs.resize(want.size() * nsubc);
        nns.resize(want.size() * nsubc);
        HIP_TRY(hipMemcpyAsync(szs.data() + first * nsubc, g, m * nsubc * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipMemcpyAsync(nns.data() + first * nsubc, g + m * nsubc, m * nsubc * sizeof(uint32_t), hipMemcpyDeviceToHost,
                               h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        return IVFHNSW_OK;
    };
    auto need = [&](uint32_t c) {
        if (at.emplace(c, want.size()).second)
            want.push_back(c);
    };
    for (size_t c = 0; c < nc; c += step)
        need((uint32_t)c);
    if ((rc = fetch(0)))
        return rc;
    const size_t sampled = want.size();
    for (size_t i = 0; i < sampled; i++)
        for (size_t j = 0; j < take; j++)
            if (nns[i * nsubc + j] < nc)
                need(nns[i * nsubc + j]);
    if ((rc = fetch(sampled)))
        return rc;
    *dedupe = grouping_dedupe_rows(nc, nsubc, [&](size_t c) { return szs.data() + at.at((uint32_t)c) * nsubc; },
                                   [&](size_t c) { return nns.data() + at.at((uint32_t)c) * nsubc; });
    return IVFHNSW_OK;
}

} // namespace ivfhnsw_gpu_impl

int ivfhnsw_gpu_upload_ivf(ivfhnsw_gpu *h, const ivfhnsw_ivf_desc *d)
try {
    int rc = table_change_guard(h, kUploads, "upload_ivf", false);
    if (rc)
        return rc;
    uint64_t n_local = 0;
    if ((rc = upload_tables(h, d, true, n_local)))
        return rc;
    if ((rc = upload(h->codes, d->codes, n_local * d->code_size)))
        return rc;
    if ((rc = upload(h->ncodes, d->norm_codes, n_local)))
        return rc;
    if ((rc = upload(h->ids, d->ids, n_local * sizeof(uint32_t))))
        return rc;
    point_at_lists(h, n_local);
    h->has_ivf = true;
    h->has_group = false;
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "ivfhnsw_gpu_upload_ivf: host allocation failed");
}

int ivfhnsw_gpu_upload_ivf_synthetic(ivfhnsw_gpu *h, const ivfhnsw_ivf_desc *d, uint64_t seed)
try {
    int rc = table_change_guard(h, kUploads, "upload_ivf_synthetic", false);
    if (rc)
        return rc;
    uint64_t n_local = 0;
    if ((rc = upload_tables(h, d, false, n_local)))
        return rc;
    if ((rc = h->codes.ensure(n_local * d->code_size)))
        return rc;
    if ((rc = h->ncodes.ensure(n_local)))
        return rc;
    if ((rc = h->ids.ensure(n_local * sizeof(uint32_t))))
        return rc;
    if (d->offsets[d->nc] > 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "synthetic corpus: more than 2^32 vectors (ids are uint32)");
    HIP_TRY(launch_fill_lists(h->stream, h->t, h->codes.as<uint8_t>(), h->ncodes.as<uint8_t>(), h->ids.as<uint32_t>(),
                              seed, seed ^ 0x6e6f726d6e6f726dull));
    HIP_TRY(hipStreamSynchronize(h->stream));
    point_at_lists(h, n_local);
    h->has_ivf = true;
    h->has_group = false;
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "ivfhnsw_gpu_upload_ivf_synthetic: host allocation failed");
}

// How much do the neighbour lists of groups a query probes together overlap?  Sampled: a group and its 15 nearest
// neighbour groups stand for a query's probes; the share of DISTINCT ids in their 16 lists.  Clustered centroids
// (k-means of real descriptors): ~0.1-0.3, the plan's hash set saves most row gathers; iid synthetic: ~0.7, it costs
// more than it saves (measured).  Tables [nc * nsubc]; upload_grouping sets g.dedupe by it (updates in place: grouping_dedupe_dev).
static int grouping_dedupe(size_t nc, size_t nsubc, const uint32_t *subgroup_sizes, const uint32_t *nn_centroid_idxs)
{
    return grouping_dedupe_rows(nc, nsubc, [&](size_t c) { return subgroup_sizes + c * nsubc; },
                                [&](size_t c) { return nn_centroid_idxs + c * nsubc; });
}

int ivfhnsw_gpu_upload_grouping(ivfhnsw_gpu *h, size_t nsubc, const float *alphas, const uint32_t *nn_centroid_idxs,
                                const uint32_t *subgroup_sizes, const float *inter_centroid_dists)
try {
    int rc = table_change_guard(h, kUploads, "upload_grouping", true);
    if (rc)
        return rc;
    if (nsubc == 0 || nsubc > 4096 || !alphas || !nn_centroid_idxs || !subgroup_sizes || !inter_centroid_dists)
        return fail(IVFHNSW_ERR_INVALID, "bad grouping tables (nsubc %zu)", nsubc);
    const size_t nc = h->t.nc;
    // every group's sub-group sizes must add up to the list size, and neighbours must be valid ids
    {
        std::vector<uint64_t> goff(nc + 1);
        HIP_TRY(hipMemcpy(goff.data(), h->goff.p, (nc + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (size_t c = 0; c < nc; c++) {
            uint64_t s = 0;
            for (size_t j = 0; j < nsubc; j++) {
                s += subgroup_sizes[c * nsubc + j];
                if (subgroup_sizes[c * nsubc + j] && nn_centroid_idxs[c * nsubc + j] >= nc)
                    return fail(IVFHNSW_ERR_INVALID, "nn_centroid_idxs[%zu][%zu] out of range", c, j);
            }
            if (s != goff[c + 1] - goff[c])
                return fail(IVFHNSW_ERR_INVALID, "subgroup sizes of list %zu sum to %llu, list holds %llu", c,
                            (unsigned long long)s, (unsigned long long)(goff[c + 1] - goff[c]));
        }
    }
    if ((rc = upload(h->g_alpha, alphas, nc * sizeof(float))))
        return rc;
    if ((rc = upload(h->g_nn, nn_centroid_idxs, nc * nsubc * sizeof(uint32_t))))
        return rc;
    if ((rc = upload(h->g_sizes, subgroup_sizes, nc * nsubc * sizeof(uint32_t))))
        return rc;
    if ((rc = upload(h->g_inter, inter_centroid_dists, nc * nsubc * sizeof(float))))
        return rc;
    h->g.nsubc = (int)nsubc;
    h->g.alphas = h->g_alpha.as<float>();
    h->g.nn_idx = h->g_nn.as<uint32_t>();
    h->g.sub_sizes = h->g_sizes.as<uint32_t>();
    h->g.inter_dists = h->g_inter.as<float>();
    h->g.dedupe = grouping_dedupe(nc, nsubc, subgroup_sizes, nn_centroid_idxs);
    h->has_group = true;
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "ivfhnsw_gpu_upload_grouping: host allocation failed");
}

// The walk's exact rejection filter (kernels_hnsw.hip): one byte per component, x ~ lo + step * byte with one
// (lo, step) for the whole table, and the largest row error ||x - (lo + step*byte)|| in units of step, rounded
// up -- and every row's own error as a 9-bit code in steps of 1/511 of the largest (walk_bound.h), which the
// neighbour rows' norm table carries to the walk.  Tables with non-finite values, a single value or d > 2048 run
// without the filter (always exact, only slower); IVFHNSW_WALK_PREFILTER=0 turns it off for A/B runs.
static int build_byte_rows(ivfhnsw_gpu *h, size_t n, size_t d, const float *vectors)
{
    static const bool off = [] {
        const char *e = getenv("IVFHNSW_WALK_PREFILTER");
        return e && atoi(e) == 0;
    }();
    if (off || d > 2048)
        return IVFHNSW_OK;
    float lo = vectors[0], hi = vectors[0];
    bool finite = true;
    for (size_t i = 0; i < n * d; i++) {
        const float v = vectors[i];
        finite &= std::isfinite(v);
        lo = std::min(lo, v);
        hi = std::max(hi, v);
    }
    const float step = (float)(((double)hi - (double)lo) / 255.0);
    if (!finite || !(step > 0.f) || !std::isfinite(step) || !std::isfinite(1.f / step))
        return IVFHNSW_OK;
    std::vector<uint8_t> rows(n * d);
    double worst = 0.0;
    std::vector<double> row_e2(n);
    for (size_t r = 0; r < n; r++) {
        double e2 = 0.0;
        for (size_t j = 0; j < d; j++) {
            const double x = vectors[r * d + j];
            double c = std::nearbyint((x - (double)lo) / (double)step);
            c = std::min(255.0, std::max(0.0, c));
            rows[r * d + j] = (uint8_t)c;
            const double e = x - ((double)lo + (double)step * c);
            e2 += e * e;
        }
        row_e2[r] = e2;
        worst = std::max(worst, e2);
    }
    const double errc = walk_err_round_up(worst, (double)step);
    float errc_f = (float)errc;
    if ((double)errc_f < errc)
        errc_f = std::nextafter(errc_f, INFINITY);
    const float unit = walk_err_unit(errc_f);
    std::vector<uint16_t> codes(n);
    for (size_t r = 0; r < n; r++)
        codes[r] = (uint16_t)walk_err_code(walk_err_round_up(row_e2[r], (double)step), unit);
    int rc = upload(h->q_qrows, rows.data(), n * d);
    if (rc)
        return rc;
    if ((rc = upload(h->q_rowerr, codes.data(), n * sizeof(uint16_t))))
        return rc;
    h->gr.qrows = h->q_qrows.as<uint8_t>();
    h->gr.q_lo = lo;
    h->gr.q_step = step;
    h->gr.q_errc = errc_f;
    h->gr.q_errunit = unit;
    return IVFHNSW_OK;
}

// Second copy of the byte rows in walk order (GraphTables::nbrows): 128 B per link, so n * maxM * 128 bytes --
// 4 GiB for the reference's 993127-centroid, maxM 32 quantizer.  Skipped (the walk then gathers from qrows)
// for d > 128, above IVFHNSW_WALK_NBROWS_GIB (default 48) and with IVFHNSW_WALK_PREFILTER=1.
static int build_neighbour_rows(ivfhnsw_gpu *h)
{
    static const int mode = [] {
        const char *e = getenv("IVFHNSW_WALK_PREFILTER");
        return e ? atoi(e) : 2;
    }();
    static const double cap_gib = [] {
        const char *e = getenv("IVFHNSW_WALK_NBROWS_GIB");
        return e ? atof(e) : 48.0;
    }();
    if (!h->gr.qrows || mode != 2 || h->gr.d > 128 || h->gr.n >= (1u << 24) || h->gr.maxM > 64)
        return IVFHNSW_OK;
    const int nb_rows = (h->gr.maxM + 31) & ~31;
    const size_t bytes = (size_t)h->gr.n * nb_rows * 128;
    if ((double)bytes > cap_gib * 1073741824.0)
        return IVFHNSW_OK;
    int rc = h->q_nbrows.ensure(bytes);
    if (rc)
        return rc;
    if ((rc = h->q_nbnorms.ensure((size_t)h->gr.n * nb_rows * sizeof(uint32_t))))
        return rc;
    if ((rc = h->q_links_c.ensure((size_t)h->gr.n * h->gr.maxM * sizeof(uint32_t))))
        return rc;
    HIP_TRY(launch_build_nbrows(h->stream, h->gr, h->q_nbrows.as<uint8_t>(), h->q_nbnorms.as<uint32_t>(), nb_rows,
                                h->q_links_c.as<uint32_t>(), h->q_rowerr.as<uint16_t>()));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->gr.nbrows = h->q_nbrows.as<uint8_t>();
    h->gr.nbnorms = h->q_nbnorms.as<uint32_t>();
    h->gr.links_c = h->q_links_c.as<uint32_t>();
    h->gr.nb_rows = nb_rows;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_upload_quantizer(ivfhnsw_gpu *h, size_t n, size_t d, size_t maxM, uint32_t enterpoint,
                                 const uint8_t *link_counts, const uint32_t *links, const float *vectors)
try {
    int rc = table_change_guard(h, kUploads, "upload_quantizer", false);
    if (rc)
        return rc;
    if (n == 0 || d == 0 || maxM == 0 || maxM > 255 || n >= 0xffffffffull || enterpoint >= n || !link_counts ||
        !links || !vectors)
        return fail(IVFHNSW_ERR_INVALID, "bad quantizer arrays (n %zu, d %zu, maxM %zu)", n, d, maxM);
    if (d % 16)
        return fail(IVFHNSW_ERR_INVALID, "d %zu: the reference distance ignores dims beyond a multiple of 16 "
                                         "(hnswalg.cpp:330); only multiples of 16 are supported here", d);
    // Link lists without repeated ids (every graph the reference builds) is what the walk's visited set assumes
    // (kernels_hnsw.hip, VisFields).  A repeated id has no effect in the reference -- the second occurrence is
    // skipped as visited (hnswalg.cpp:80-82) -- so lists that have them are uploaded without the repeats.
    bool unique = true;
    uint32_t tmp[256];
    for (size_t i = 0; i < n; i++) {
        if (link_counts[i] > maxM)
            return fail(IVFHNSW_ERR_INVALID, "node %zu has %u links > maxM %zu", i, link_counts[i], maxM);
        for (size_t j = 0; j < link_counts[i]; j++)
            if (links[i * maxM + j] >= n)
                return fail(IVFHNSW_ERR_INVALID, "node %zu link %zu out of range", i, j);
        if (unique && link_counts[i] > 1) {
            const size_t c = link_counts[i];
            std::copy(links + i * maxM, links + i * maxM + c, tmp);
            std::sort(tmp, tmp + c);
            unique = std::adjacent_find(tmp, tmp + c) == tmp + c;
        }
    }
    std::vector<uint8_t> counts_u;
    std::vector<uint32_t> links_u;
    if (!unique) {
        counts_u.assign(link_counts, link_counts + n);
        links_u.assign(links, links + n * maxM);
        for (size_t i = 0; i < n; i++) {
            uint32_t *row = links_u.data() + i * maxM;
            size_t c = 0;
            for (size_t j = 0; j < link_counts[i]; j++) {
                bool seen = false;
                for (size_t k2 = 0; k2 < c && !seen; k2++)
                    seen = row[k2] == row[j];
                if (!seen)
                    row[c++] = row[j];
            }
            for (size_t j = c; j < link_counts[i]; j++)
                row[j] = 0;
            counts_u[i] = (uint8_t)c;
        }
        link_counts = counts_u.data();
        links = links_u.data();
        unique = true;
    }
    if ((rc = upload(h->q_counts, link_counts, n)))
        return rc;
    if ((rc = upload(h->q_links, links, n * maxM * sizeof(uint32_t))))
        return rc;
    if ((rc = upload(h->q_vectors, vectors, n * d * sizeof(float))))
        return rc;
    h->gr.n = (uint32_t)n;
    h->gr.d = (int)d;
    h->gr.maxM = (int)maxM;
    h->gr.enterpoint = enterpoint;
    h->gr.counts = h->q_counts.as<uint8_t>();
    h->gr.links = h->q_links.as<uint32_t>();
    h->gr.vectors = h->q_vectors.as<float>();
    {
        static const int merge = [] {
            const char *e = getenv("IVFHNSW_WALK_MERGE");
            return (e && atoi(e) == 0) ? 0 : 1;
        }();
        h->gr.merge_admissions = merge;
    }
    {
        // IVFHNSW_WALK_LATE_VISIT: 1 always, 0 never, unset = where it pays -- graphs whose ids need more than 8 tag
        // bits (walk_late_visit_default, walk_form.h), where the visited set of a query would otherwise run 40 % full and
        // overflow into global atomics (1.60 -> 1.50 ms per 10 k queries at 993 127 nodes; at 2^17 nodes the extra
        // LDS pass costs 1 %: 1.19 -> 1.205 ms)
        static const int late_knob = [] {
            const char *e = getenv("IVFHNSW_WALK_LATE_VISIT");
            return e ? (atoi(e) != 0 ? 1 : 0) : -1;
        }();
        const bool late = late_knob < 0 ? walk_late_visit_default(n) : late_knob == 1;
        h->gr.links_unique = (unique && late) ? 1 : 0;
    }
    h->gr.fat = nullptr; // the latency form's copy belongs to the previous graph
    h->gr.qrows = nullptr;
    h->gr.nbrows = nullptr;
    h->gr.nbnorms = nullptr;
    h->gr.links_c = nullptr;
    h->gr.nb_rows = 0;
    h->gr.q_lo = 0.f;
    h->gr.q_step = 1.f;
    h->gr.q_errc = 0.f;
    h->gr.q_errunit = 0.f;
    if ((rc = build_byte_rows(h, n, d, vectors)))
        return rc;
    if ((rc = build_neighbour_rows(h)))
        return rc;
    h->has_graph = true;
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "ivfhnsw_gpu_upload_quantizer: host allocation failed");
}

int ivfhnsw_gpu_prepare_latency(ivfhnsw_gpu *h)
{
    if (h && h->is_view)
        return fail(IVFHNSW_ERR_STATE, "prepare_latency goes to the handle that holds the tables, not to a view of it");
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "prepare_latency needs upload_quantizer");
    if (h->gr.fat)
        return IVFHNSW_OK;
    GraphTables probe = h->gr;
    probe.fat = reinterpret_cast<const float *>(h); // any non-null value: shape check only
    if (!coarse_latency_supported(probe, 1))
        return fail(IVFHNSW_ERR_INVALID, "the latency walk needs d = 128 or 96, maxM <= 32 and at most 2^20 nodes "
                                         "(have d %d, maxM %d, %u nodes); small batches keep the throughput walk",
                    h->gr.d, h->gr.maxM, h->gr.n);
    if ((rc = h->q_fat.ensure(coarse_latency_fat_bytes(h->gr))))
        return rc;
    HIP_TRY(launch_build_fat(h->stream, h->gr, h->q_fat.as<float>()));
    HIP_TRY(hipStreamSynchronize(h->stream));
    h->gr.fat = h->q_fat.as<float>();
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_download_grouping_tables(ivfhnsw_gpu *h, float *alphas, uint32_t *nn_centroid_idxs, uint32_t *subgroup_sizes,
                                         float *inter_centroid_dists)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_group)
        return fail(IVFHNSW_ERR_STATE, "download_grouping_tables: the handle holds no grouping tables");
    const size_t nc = h->t.nc, nsub = nc * (size_t)h->g.nsubc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (alphas)
        HIP_TRY(hipMemcpy(alphas, h->g.alphas, nc * sizeof(float), hipMemcpyDeviceToHost));
    if (nn_centroid_idxs)
        HIP_TRY(hipMemcpy(nn_centroid_idxs, h->g.nn_idx, nsub * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (subgroup_sizes)
        HIP_TRY(hipMemcpy(subgroup_sizes, h->g.sub_sizes, nsub * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (inter_centroid_dists)
        HIP_TRY(hipMemcpy(inter_centroid_dists, h->g.inter_dists, nsub * sizeof(float), hipMemcpyDeviceToHost));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_upload_centroid_norms(ivfhnsw_gpu *h, const float *centroid_norms)
{
    int rc = table_change_guard(h, kUploads, "upload_centroid_norms", true);
    if (rc)
        return rc;
    if (!centroid_norms)
        return fail(IVFHNSW_ERR_INVALID, "upload_centroid_norms: null buffer");
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(h->cnorm.p, centroid_norms, (size_t)h->t.nc * sizeof(float), hipMemcpyHostToDevice));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_download_ivf(ivfhnsw_gpu *h, uint64_t *offsets, uint32_t *ids, uint8_t *codes, uint8_t *norm_codes)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "download_ivf before upload_ivf");
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (offsets)
        HIP_TRY(hipMemcpy(offsets, h->t.goff, ((size_t)h->t.nc + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
    if (ids && h->n_local)
        HIP_TRY(hipMemcpy(ids, h->t.ids, h->n_local * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (codes && h->n_local)
        HIP_TRY(hipMemcpy(codes, h->t.codes, h->n_local * h->t.M, hipMemcpyDeviceToHost));
    if (norm_codes && h->n_local)
        HIP_TRY(hipMemcpy(norm_codes, h->t.norm_codes, h->n_local, hipMemcpyDeviceToHost));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_download_grouping(ivfhnsw_gpu *h, uint32_t *subgroup_sizes)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_group)
        return fail(IVFHNSW_ERR_STATE, "download_grouping: the handle holds no grouping tables");
    if (!subgroup_sizes)
        return fail(IVFHNSW_ERR_INVALID, "download_grouping: null buffer");
    HIP_TRY(hipStreamSynchronize(h->stream));
    HIP_TRY(hipMemcpy(subgroup_sizes, h->g.sub_sizes, (size_t)h->t.nc * h->g.nsubc * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return IVFHNSW_OK;
}
