// Range search (faiss's range_search): every code the k-search of the same call would score whose
// distance is below the radius.  rotate -> coarse -> plan -> table are the stages of a search_dev chunk (capi_search.cpp),
// then count -> prefix -> (one synchronisation: the host sizes the results) -> fill (kernels_range.hip).
#include "capi_internal.h"

namespace ivfhnsw_gpu_impl {

void range_drop(ivfhnsw_gpu *h)
{
    h->rg_valid = false;
    h->rg_total = 0;
    h->rg_dist.release();
    h->rg_lab.release();
}

} // namespace ivfhnsw_gpu_impl

// what both forms check before they touch anything
static int range_args_guard(ivfhnsw_gpu *h, size_t nq, const void *queries, const void *coarse_ids, const void *coarse_dists,
                            const ivfhnsw_search_params *p, float radius, const void *lims, const void *total)
{
    int rc = bind(h);
    if (rc || (rc = search_args_guard(h, p, 1)))
        return rc;
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "range_search on a sharded handle (shard_world %u): not supported", h->t.shard_world);
    if (std::isnan(radius))
        return fail(IVFHNSW_ERR_INVALID, "range_search: the radius is NaN");
    if ((coarse_ids == nullptr) != (coarse_dists == nullptr))
        return fail(IVFHNSW_ERR_INVALID, "coarse_ids and coarse_dists must both be given or both be NULL");
    if (nq > 0 && (!queries || !lims || !total))
        return fail(IVFHNSW_ERR_INVALID, "range_search: null queries, lims or total");
    if (nq > kMaxBatchAll)
        return fail(IVFHNSW_ERR_INVALID, "range_search is limited to %zu queries per call", kMaxBatchAll);
    return IVFHNSW_OK;
}

// the second pass and the wait for it; lims last, so that a refused batch leaves the caller's array alone
static int range_fill_pass(ivfhnsw_gpu *h, const Chunk &c, int seg_hint, float radius, uint64_t total, float *dist,
                           int64_t *labels, uint64_t *d_lims)
{
    HIP_TRY(launch_range_lims(h->stream, h->rg_slices.as<uint32_t>(), (int)c.nq, c.nsplit, d_lims));
    if (total) {
        StageScope sc(h, IVFHNSW_STAGE_SELECT); // the fill pass is accounted as the select stage, the count pass as the scan
        HIP_TRY(launch_range_fill(h->stream, h->t, h->w_luts.as<float>(), plan_of(h, c.max_seg, c.nq), c.nsplit, seg_hint,
                                  radius, h->rg_slices.as<uint32_t>(), dist, labels, c.fmask));
    }
    HIP_TRY(hipStreamSynchronize(h->stream));
    return check_status(h);
}

// ivfhnsw_gpu_range_search_dev, and with a pick (a slot byte, a tag or an interval per query, device memory) its _slots / _tags / _values form
static int range_search_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                            const float *d_coarse_dists, const ivfhnsw_search_params *p, const QueryPick &pick,
                            float radius, uint64_t *d_lims, uint64_t *total)
{
    int rc = range_args_guard(h, nq, d_queries, d_coarse_ids, d_coarse_dists, p, radius, d_lims, total);
    if (rc || (pick && (rc = slots_call_guard(h, pick.who("range_search_slots_dev", "range_search_tags_dev", "range_search_values_dev", "range_search_tags_values_dev"), pick.kind()))))
        return rc;
    if ((uintptr_t)pick.tags & 1)
        return fail(IVFHNSW_ERR_INVALID, "%s: query tags must be 2-byte aligned", pick.who("", "range_search_tags_dev", "", "range_search_tags_values_dev"));
    if ((uintptr_t)pick.ranges & 7)
        return fail(IVFHNSW_ERR_INVALID, "%s: query ranges must be 8-byte aligned", pick.who("", "", "range_search_values_dev", "range_search_tags_values_dev"));
    if (nq == 0) {
        if (d_lims) {
            HIP_TRY(hipMemsetAsync(d_lims, 0, sizeof(uint64_t), h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        if (total)
            *total = 0;
        h->rg_valid = true;
        h->rg_total = 0;
        return IVFHNSW_OK;
    }
    Chunk c{SearchArgs{nq, 1, d_queries, d_coarse_ids, d_coarse_dists, p, nullptr, nullptr, nullptr, pick}};
    if ((rc = chunk_checks(h, c, false)))
        return rc;
    // the workspace is about to hold this call's plan: whatever the last search left there is gone
    h->last_nq = 0;
    h->last_stream = false;
    h->last_split = false;
    h->last_parts[0] = nq;
    h->last_parts[1] = 0;
    SearchCall call;
    if ((rc = chunk_workspace(h, c)) || (rc = chunk_coarse(h, c, call)) || (rc = chunk_plan_table(h, c)))
        return rc;
    if (c.pipe) { // (a forced scan_pipe: chunk_plan_table left the table to that kernel)
        if ((rc = h->w_luts.ensure(nq * (size_t)h->t.M * 256 * sizeof(float))))
            return rc;
        StageScope sc(h, IVFHNSW_STAGE_LUT);
        HIP_TRY(launch_lut(h->stream, h->t, c.xq, h->w_luts.as<float>(), (int)nq, h->w_hdr.as<PlanHdr>()));
    }
    // a plan segment is a list (IVFADC) or a sub-group (Grouping): the mean length decides the scan form, as in search_dev
    const uint64_t nseg_all = (uint64_t)h->t.nc * (h->has_group ? (uint64_t)h->g.nsubc : 1);
    const int seg_hint = (int)std::min<uint64_t>(1u << 20, nseg_all ? h->n_local / nseg_all : 0);
    const size_t len = nq * (size_t)c.nsplit + 1;
    if ((rc = h->rg_slices.ensure(len * sizeof(uint32_t))) ||
        (rc = h->rg_part.ensure(append_scan_parts(len) * sizeof(uint32_t))))
        return rc;
    uint32_t *slices = h->rg_slices.as<uint32_t>();
    unsigned long long *d_total = h->w_totals.as<unsigned long long>();
    const char *kernel_name = "";
    {
        StageScope sc(h, IVFHNSW_STAGE_SCAN);
        HIP_TRY(launch_range_count(h->stream, h->t, h->w_luts.as<float>(), plan_of(h, c.max_seg, nq), c.nsplit, seg_hint,
                                   radius, slices, d_total, c.fmask, &kernel_name));
    }
    HIP_TRY(launch_scan_excl_u32(h->stream, slices, len, h->rg_part.as<uint32_t>()));
    // the one synchronisation between the passes: the host sizes the results from the count
    unsigned long long tot = 0;
    HIP_TRY(hipMemcpyAsync(&tot, d_total, sizeof(tot), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    // the plan in the workspace is this call's: last_scan_counts reads it, resolve_keys and last_stream do not
    h->last_scan_kernel = kernel_name;
    h->last_nq = (int)nq;
    h->last_max_seg = c.max_seg;
    h->last_range = true;
    if ((rc = check_status(h)))
        return rc;
    if (tot >= (1ull << 32))
        return fail(IVFHNSW_ERR_INVALID, "range_search: %llu results in one batch, the limit is 2^32 - 1 (use a smaller radius or "
                                         "fewer queries per call)", tot);
    // results: in the buffers the handle holds when they are large enough, else in new ones swapped in when they are full
    DevBuf nd, nl;
    const bool grow = tot * sizeof(float) > h->rg_dist.bytes || tot * sizeof(int64_t) > h->rg_lab.bytes;
    if (grow && ((rc = nd.ensure(tot * sizeof(float))) || (rc = nl.ensure(tot * sizeof(int64_t))))) {
        nd.release();
        nl.release();
        return rc;
    }
    rc = range_fill_pass(h, c, seg_hint, radius, tot, grow ? nd.as<float>() : h->rg_dist.as<float>(),
                         grow ? nl.as<int64_t>() : h->rg_lab.as<int64_t>(), d_lims);
    if (rc) {
        nd.release();
        nl.release();
        return rc;
    }
    if (grow) {
        std::swap(h->rg_dist, nd);
        std::swap(h->rg_lab, nl);
        nd.release();
        nl.release();
    }
    h->rg_valid = true;
    h->rg_total = tot;
    *total = tot;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_range_search_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                 const float *d_coarse_dists, const ivfhnsw_search_params *p, float radius, uint64_t *d_lims,
                                 uint64_t *total)
{
    return range_search_dev(h, nq, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{}, radius, d_lims, total);
}

int ivfhnsw_gpu_range_search_slots_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                       const float *d_coarse_dists, const ivfhnsw_search_params *p,
                                       const uint8_t *d_query_slots, float radius, uint64_t *d_lims, uint64_t *total)
{
    return range_search_dev(h, nq, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{d_query_slots, nullptr}, radius, d_lims,
                            total);
}

int ivfhnsw_gpu_range_search_tags_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                      const float *d_coarse_dists, const ivfhnsw_search_params *p,
                                      const uint16_t *d_query_tags, float radius, uint64_t *d_lims, uint64_t *total)
{
    return range_search_dev(h, nq, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{nullptr, d_query_tags}, radius, d_lims,
                            total);
}

int ivfhnsw_gpu_range_search_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                        const float *d_coarse_dists, const ivfhnsw_search_params *p,
                                        const uint32_t *d_query_ranges, float radius, uint64_t *d_lims, uint64_t *total)
{
    return range_search_dev(h, nq, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{nullptr, nullptr, d_query_ranges}, radius,
                            d_lims, total);
}

int ivfhnsw_gpu_range_search_tags_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                             const float *d_coarse_dists, const ivfhnsw_search_params *p,
                                             const uint16_t *d_query_tags, const uint32_t *d_query_ranges, float radius,
                                             uint64_t *d_lims, uint64_t *total)
{
    return range_search_dev(h, nq, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{nullptr, d_query_tags, d_query_ranges},
                            radius, d_lims, total);
}

// ivfhnsw_gpu_range_search, and with a pick (host memory) ivfhnsw_gpu_range_search_slots / _tags / _values
static int range_search_host(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                             const float *coarse_dists, const ivfhnsw_search_params *p, const QueryPick &pick, float radius,
                             uint64_t *lims, uint64_t *total)
{
    int rc = range_args_guard(h, nq, queries, coarse_ids, coarse_dists, p, radius, lims, total);
    const char *who = pick.who("range_search_slots", "range_search_tags", "range_search_values", "range_search_tags_values");
    if (rc || (pick && ((rc = slots_call_guard(h, who, pick.kind())) ||
                        (pick.slots && (rc = slots_bytes_guard(nq, pick.slots, who))))))
        return rc;
    if (nq == 0) {
        if (lims)
            lims[0] = 0;
        return ivfhnsw_gpu_range_search_dev(h, 0, nullptr, nullptr, nullptr, p, radius, nullptr, total);
    }
    const size_t in_q = nq * h->t.d * sizeof(float), in_c = coarse_ids ? nq * p->nprobe * sizeof(uint32_t) : 0;
    if ((rc = h->rg_lims.ensure((nq + 1) * sizeof(uint64_t))) || (rc = stage_in(h, h->s_q, queries, in_q)) ||
        (coarse_ids && ((rc = stage_in(h, h->s_cid, coarse_ids, in_c)) || (rc = stage_in(h, h->s_cd, coarse_dists, in_c)))) ||
        (pick && (rc = pick_stage_in(h, pick, nq))) ||
        (rc = range_search_dev(h, nq, h->s_q.as<float>(), coarse_ids ? h->s_cid.as<uint32_t>() : nullptr,
                               coarse_ids ? h->s_cd.as<float>() : nullptr, p, pick.at(h->fs_qslots.p, nq),
                               radius, h->rg_lims.as<uint64_t>(), total)) ||
        (rc = stage_out(h, lims, h->rg_lims, (nq + 1) * sizeof(uint64_t))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_range_search(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                             const float *coarse_dists, const ivfhnsw_search_params *p, float radius, uint64_t *lims,
                             uint64_t *total)
{
    return range_search_host(h, nq, queries, coarse_ids, coarse_dists, p, QueryPick{}, radius, lims, total);
}

int ivfhnsw_gpu_range_search_slots(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                   const float *coarse_dists, const ivfhnsw_search_params *p, const uint8_t *query_slots,
                                   float radius, uint64_t *lims, uint64_t *total)
{
    return range_search_host(h, nq, queries, coarse_ids, coarse_dists, p, QueryPick{query_slots, nullptr}, radius, lims, total);
}

int ivfhnsw_gpu_range_search_tags(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                  const float *coarse_dists, const ivfhnsw_search_params *p, const uint16_t *query_tags,
                                  float radius, uint64_t *lims, uint64_t *total)
{
    return range_search_host(h, nq, queries, coarse_ids, coarse_dists, p, QueryPick{nullptr, query_tags}, radius, lims, total);
}

int ivfhnsw_gpu_range_search_values(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                    const float *coarse_dists, const ivfhnsw_search_params *p, const uint32_t *query_ranges,
                                    float radius, uint64_t *lims, uint64_t *total)
{
    return range_search_host(h, nq, queries, coarse_ids, coarse_dists, p, QueryPick{nullptr, nullptr, query_ranges}, radius, lims, total);
}

int ivfhnsw_gpu_range_search_tags_values(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                         const float *coarse_dists, const ivfhnsw_search_params *p, const uint16_t *query_tags,
                                         const uint32_t *query_ranges, float radius, uint64_t *lims, uint64_t *total)
{
    return range_search_host(h, nq, queries, coarse_ids, coarse_dists, p, QueryPick{nullptr, query_tags, query_ranges}, radius, lims,
                             total);
}

int ivfhnsw_gpu_range_results(ivfhnsw_gpu *h, uint64_t first, uint64_t count, float *distances, int64_t *labels)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->rg_valid)
        return fail(IVFHNSW_ERR_STATE, "range_results before a range search on this handle");
    if (first > h->rg_total || count > h->rg_total - first)
        return fail(IVFHNSW_ERR_INVALID, "range_results: [%llu, %llu + %llu) is beyond the %llu results held",
                    (unsigned long long)first, (unsigned long long)first, (unsigned long long)count,
                    (unsigned long long)h->rg_total);
    if (count == 0)
        return IVFHNSW_OK;
    if (distances)
        HIP_TRY(hipMemcpyAsync(distances, h->rg_dist.as<float>() + first, count * sizeof(float), hipMemcpyDeviceToHost, h->stream));
    if (labels)
        HIP_TRY(hipMemcpyAsync(labels, h->rg_lab.as<int64_t>() + first, count * sizeof(int64_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_range_results_dev(ivfhnsw_gpu *h, const float **d_distances, const int64_t **d_labels, uint64_t *total)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->rg_valid)
        return fail(IVFHNSW_ERR_STATE, "range_results_dev before a range search on this handle");
    if (d_distances)
        *d_distances = h->rg_total ? h->rg_dist.as<float>() : nullptr;
    if (d_labels)
        *d_labels = h->rg_total ? h->rg_lab.as<int64_t>() : nullptr;
    if (total)
        *total = h->rg_total;
    return IVFHNSW_OK;
}
