// In-place updates of the resident lists: appends, additions to a Grouping index (3.12), removals (3.11),
// upserts (3.23).
#include "capi_internal.h"

// ---------------------------------------------------------------------------------------------------------------
// what the three cores share

// (run_with_word, one device word as a kernel's answer: capi_labels.cpp)

// The tail of an update, behind the last launch that fills `fresh` (e = the launches' status): the stream is drained,
// the handle's filter is judged over the new ids, and only then do the new arrays replace the old ones -- every error up
// to that point leaves the handle's tables the ones it had.  new_sizes (Grouping handles; null otherwise) = the staging
// that holds the new sub-group sizes: the choice upload_grouping derives from the sizes and the neighbour rows follows
// them (its workspace was reserved by the caller, grouping_dedupe_reserve, before the first new byte was written), and
// the staging becomes the table, the old table the next call's staging.
static int commit_lists(ivfhnsw_gpu *h, const char *who, hipError_t e, ListArrays &fresh, uint64_t n_local2, DevBuf *new_sizes)
{
    if (e == hipSuccess)
        e = hipStreamSynchronize(h->stream);
    if (e != hipSuccess)
        return fail(e == hipErrorOutOfMemory ? IVFHNSW_ERR_NOMEM : IVFHNSW_ERR_HIP, "%s: %s", who, hipGetErrorString(e));
    int rc, dedupe = h->g.dedupe;
    if (new_sizes && (rc = grouping_dedupe_dev(h, new_sizes->as<uint32_t>(), h->g.nn_idx, &dedupe)))
        return rc;
    if ((rc = fresh.mark_filter(h, n_local2)))
        return rc;
    fresh.install(h, n_local2);
    if (new_sizes) {
        std::swap(h->g_sizes, *new_sizes);
        h->g.sub_sizes = h->g_sizes.as<uint32_t>();
        h->g.dedupe = dedupe;
    }
    return IVFHNSW_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// appends to the lists the handle holds: the new CSR is built beside the old one and swapped in
static int append_state(ivfhnsw_gpu *h, const char *who)
{
    int rc = table_change_guard(h, kAppends, who, true);
    if (rc)
        return rc;
    if (h->has_group)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle holds grouping tables, whose lists have no append", who);
    return IVFHNSW_OK;
}

static int append_size(ivfhnsw_gpu *h, size_t n, const char *who)
{
    if (n >= 0xffffffffull || h->n_local + n >= 0xffffffffull)
        return fail(IVFHNSW_ERR_INVALID, "%s: %llu + %zu codes reach 2^32 - 1 on one shard", who,
                    (unsigned long long)h->n_local, n);
    return IVFHNSW_OK;
}

// the batch's staging in HBM: list ids, ids, codes, norm codes of n rows
static int append_stage(ivfhnsw_gpu *h, size_t n)
{
    int rc;
    if ((rc = h->ap_idx.ensure(n * sizeof(uint32_t))) || (rc = h->ap_ids.ensure(n * sizeof(uint32_t))) ||
        (rc = h->ap_codes.ensure(n * h->t.M)) || (rc = h->ap_ncodes.ensure(n)))
        return rc;
    return IVFHNSW_OK;
}

// a host batch into the staging (sub_idx null: IVFADC lists)
static int stage_batch(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *sub_idx, const uint32_t *ids,
                       const uint8_t *codes, const uint8_t *norm_codes)
{
    int rc;
    if ((rc = append_stage(h, n)) || (sub_idx && (rc = h->gp_sub.ensure(n * sizeof(uint32_t)))))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->ap_idx.p, list_idx, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    if (sub_idx)
        HIP_TRY(hipMemcpyAsync(h->gp_sub.p, sub_idx, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ap_ids.p, ids, n * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ap_codes.p, codes, n * h->t.M, hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ap_ncodes.p, norm_codes, n, hipMemcpyHostToDevice, h->stream));
    return IVFHNSW_OK;
}

// The first step of both append cores.  The batch's rows are counted per list, with d_sub per list and sub-group too
// (sizes2 starts as a copy of the handle's sizes), launch_append_tables scans the counts into the new lists' starts
// (ap_cnt, ap_own), and the id check's flag and the new total come to the host.  Returns with the stream drained and the
// handle's tables untouched.
static int append_count(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list, const uint32_t *d_sub, uint32_t *sizes2,
                        bool *bad_id, uint64_t *n_local2)
{
    const size_t nc = h->t.nc, len = nc + 1;
    const uint32_t nsubc = d_sub ? (uint32_t)h->g.nsubc : 0u;
    int rc;
    if ((rc = h->ap_cnt.ensure(len * sizeof(uint32_t))) || (rc = h->ap_own.ensure(len * sizeof(uint32_t))) ||
        (rc = h->ap_part.ensure(append_scan_parts(len) * sizeof(uint32_t))))
        return rc;
    uint32_t *cnt = h->ap_cnt.as<uint32_t>(), *own = h->ap_own.as<uint32_t>();
    uint32_t st = 0, total = 0;
    rc = run_with_word(h, h->ap_status, 0, [&](uint32_t *status) -> hipError_t {
        hipError_t e = hipMemsetAsync(cnt, 0, len * sizeof(uint32_t), h->stream);
        if (e == hipSuccess && d_sub)
            e = hipMemcpyAsync(sizes2, h->g.sub_sizes, nc * nsubc * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream);
        if (e == hipSuccess)
            e = launch_append_count(h->stream, d_list, d_sub, n, (uint32_t)nc, nsubc, cnt, d_sub ? sizes2 : nullptr, status);
        if (e == hipSuccess)
            e = launch_append_tables(h->stream, h->t, cnt, own, h->ap_part.as<uint32_t>());
        if (e == hipSuccess)
            e = hipMemcpyAsync(&total, own + nc, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream);
        return e;
    }, &st);
    if (rc)
        return rc;
    *bad_id = st != 0;
    *n_local2 = total;
    return IVFHNSW_OK;
}

// the sort's and the merge's workspace for a batch of n rows into lists of n_local2 codes
static int append_workspace(ivfhnsw_gpu *h, size_t n, uint64_t n_local2)
{
    const size_t nblocks = (n + kKmeansTile - 1) / kKmeansTile;
    int rc;
    if ((rc = h->ap_perm.ensure(n * sizeof(uint32_t))) || (rc = h->ap_perm2.ensure(n * sizeof(uint32_t))) ||
        (rc = h->ap_hist.ensure(256 * nblocks * sizeof(uint32_t))) ||
        (rc = h->ap_tiles.ensure(append_tile_words(n_local2, kAppendTileRows) * sizeof(uint32_t))))
        return rc;
    return IVFHNSW_OK;
}

// d_idx [n] (every id < nc is checked here, on the device, before anything changes), d_ids [n], d_codes [n][M] (dword
// aligned), d_ncodes [n]: device memory, read on the handle's stream.  Returns with the stream drained; on any error
// the handle's tables are the ones it had.
static int append_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_idx, const uint32_t *d_ids, const uint8_t *d_codes,
                       const uint8_t *d_ncodes)
{
    const size_t nc = h->t.nc;
    int rc;
    bool bad_id = false;
    uint64_t n_local2 = 0;
    if ((rc = append_count(h, n, d_idx, nullptr, nullptr, &bad_id, &n_local2)))
        return rc;
    if (bad_id)
        return fail(IVFHNSW_ERR_INVALID, "append: a list id is >= nc = %zu", nc);
    if ((rc = append_workspace(h, n, n_local2)))
        return rc;
    // the new arrays first: the old ones stay the handle's until the new ones are complete
    ListArrays fresh;
    if ((rc = fresh.allocate(nc, n_local2, h->t.M)))
        return rc;
    const NewLists nl = fresh.view(n_local2);
    uint32_t *perm = nullptr, *tiles = h->ap_tiles.as<uint32_t>();
    const uint32_t *nstart = h->ap_cnt.as<uint32_t>(), *lstart = h->ap_own.as<uint32_t>(); // scanned in place by launch_append_tables
    hipError_t e = launch_sort_by_key(h->stream, d_idx, n, bits_of(nc - 1), h->ap_perm.as<uint32_t>(),
                                      h->ap_perm2.as<uint32_t>(), h->ap_hist.as<uint32_t>(), &perm);
    if (e == hipSuccess)
        e = launch_append_layout(h->stream, h->t, nstart, lstart, tiles, nl);
    if (e == hipSuccess)
        e = launch_append_merge(h->stream, h->t, nstart, lstart, tiles, nullptr, nl);
    if (e == hipSuccess)
        e = launch_append_scatter(h->stream, h->t, perm, d_idx, n, nstart, lstart, nullptr, d_codes, d_ncodes, d_ids, nl);
    return commit_lists(h, "append", e, fresh, n_local2, nullptr);
}

int ivfhnsw_gpu_append_ivf(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *ids, const uint8_t *codes,
                           const uint8_t *norm_codes)
{
    int rc = append_state(h, "append_ivf");
    if (rc || n == 0)
        return rc;
    if (!list_idx || !ids || !codes || !norm_codes)
        return fail(IVFHNSW_ERR_INVALID, "append_ivf: null buffer");
    if ((rc = append_size(h, n, "append_ivf")))
        return rc;
    for (size_t i = 0; i < n; i++)
        if (list_idx[i] >= h->t.nc)
            return fail(IVFHNSW_ERR_INVALID, "append_ivf: list_idx[%zu] = %u, nc = %u", i, list_idx[i], h->t.nc);
    if ((rc = stage_batch(h, n, list_idx, nullptr, ids, codes, norm_codes)))
        return rc;
    return append_core(h, n, h->ap_idx.as<uint32_t>(), h->ap_ids.as<uint32_t>(), h->ap_codes.as<uint8_t>(),
                       h->ap_ncodes.as<uint8_t>());
}

int ivfhnsw_gpu_append_ivf_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list_idx, const uint32_t *d_ids,
                               const uint8_t *d_codes, const uint8_t *d_norm_codes)
{
    int rc = append_state(h, "append_ivf_dev");
    if (rc || n == 0)
        return rc;
    if (!d_list_idx || !d_ids || !d_codes || !d_norm_codes)
        return fail(IVFHNSW_ERR_INVALID, "append_ivf_dev: null buffer");
    if (((uintptr_t)d_list_idx | (uintptr_t)d_ids | (uintptr_t)d_codes) & 3)
        return fail(IVFHNSW_ERR_INVALID, "append_ivf_dev: list_idx, ids and codes must be 4-byte aligned");
    if ((rc = append_size(h, n, "append_ivf_dev")))
        return rc;
    return append_core(h, n, d_list_idx, d_ids, d_codes, d_norm_codes);
}

// what add and add_groups need beside the lists: code books and a quantizer that fit the index
static int check_add_ready(ivfhnsw_gpu *h, const char *who)
{
    if (!h->has_codebooks || !h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "%s needs upload_codebooks and upload_quantizer", who);
    if (h->gr.n != h->t.nc || h->gr.d != h->t.d)
        return fail(IVFHNSW_ERR_STATE, "%s: the quantizer holds %u x %d, the index %u lists of d = %d", who, h->gr.n,
                    h->gr.d, h->t.nc, h->t.d);
    if (h->e_d != (size_t)h->t.d || h->e_M != (size_t)h->t.M || h->e_opq != (h->t.opq_At != nullptr))
        return fail(IVFHNSW_ERR_INVALID, "%s: code books (d %zu, code_size %zu, %s OPQ) do not match the index (d %d, "
                    "code_size %d, %s OPQ)", who, h->e_d, h->e_M, h->e_opq ? "with" : "no", h->t.d, h->t.M,
                    h->t.opq_At ? "with" : "no");
    return IVFHNSW_OK;
}

static int upsert_state(ivfhnsw_gpu *h, const char *who);
static int upsert_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_idx, const uint32_t *d_ids, const uint8_t *d_codes,
                       const uint8_t *d_ncodes, uint64_t *n_removed, uint32_t *rem_out);

// encode (as ivfhnsw_gpu_encode, chunk by chunk) into the staging, then one append -- or, with n_removed (upsert: the
// codes that bore one of ids leave first, 3.23), one upsert
static int add_impl(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *pidx, size_t efSearch, const uint32_t *ids,
                    uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes, bool dev, const char *who,
                    uint64_t *n_removed = nullptr)
{
    int rc = n_removed ? upsert_state(h, who) : append_state(h, who);
    if (rc || (rc = check_add_ready(h, who)))
        return rc;
    if (n == 0)
        return IVFHNSW_OK;
    if (!x || !ids)
        return fail(IVFHNSW_ERR_INVALID, "%s: null buffer", who);
    if (!pidx && efSearch == 0)
        return fail(IVFHNSW_ERR_INVALID, "%s: efSearch 0 (assign runs searchKnn(x, 1))", who);
    if ((rc = append_size(h, n, who)))
        return rc;
    if ((rc = append_stage(h, n)))
        return rc;
    const hipMemcpyKind in = dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    const hipMemcpyKind out = dev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    uint32_t *sidx = h->ap_idx.as<uint32_t>();
    if (pidx) {
        if (!dev) {
            for (size_t i = 0; i < n; i++)
                if (pidx[i] >= h->t.nc)
                    return fail(IVFHNSW_ERR_INVALID, "%s: precomputed_idx[%zu] = %u out of range", who, i, pidx[i]);
        }
        HIP_TRY(hipMemcpyAsync(sidx, pidx, n * sizeof(uint32_t), in, h->stream));
        if (dev) { // before the encoder reads a centroid row by it
            uint32_t st = 0;
            if ((rc = run_with_word(h, h->ap_status, 0, [&](uint32_t *status) {
                     return launch_append_count(h->stream, sidx, nullptr, n, h->t.nc, 0u, nullptr, nullptr, status);
                 }, &st)))
                return rc;
            if (st)
                return fail(IVFHNSW_ERR_INVALID, "%s: a precomputed_idx is >= nc = %u", who, h->t.nc);
        }
    }
    const size_t d = h->e_d, M = h->e_M;
    const size_t kChunk = (size_t)1 << 18;
    for (size_t i0 = 0; i0 < n; i0 += kChunk) {
        const size_t m = std::min(kChunk, n - i0);
        if ((rc = h->e_x.ensure(m * d * sizeof(float))) || (rc = h->e_res.ensure(m * d * sizeof(float))) ||
            (rc = h->e_tmp.ensure(m * d * sizeof(float))) || (rc = h->e_dist.ensure(m * sizeof(float))) ||
            (rc = h->e_codes.ensure(m * M)) || (rc = h->e_ncodes.ensure(m)))
            return rc;
        float *dx = h->e_x.as<float>();
        HIP_TRY(hipMemcpyAsync(dx, x + i0 * d, m * d * sizeof(float), in, h->stream));
        if (!pidx && (rc = ivfhnsw_gpu_coarse_dev(h, m, dx, 1, efSearch, sidx + i0, h->e_dist.as<float>())))
            return rc;
        if ((rc = encode_rows(h, m, dx, h->gr.vectors, sidx + i0)))
            return rc;
        HIP_TRY(hipMemcpyAsync(h->ap_codes.as<uint8_t>() + i0 * M, h->e_codes.p, m * M, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipMemcpyAsync(h->ap_ncodes.as<uint8_t>() + i0, h->e_ncodes.p, m, hipMemcpyDeviceToDevice, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
        if ((rc = check_status(h)))
            return rc;
    }
    HIP_TRY(hipMemcpyAsync(h->ap_ids.p, ids, n * sizeof(uint32_t), in, h->stream));
    if (out_codes)
        HIP_TRY(hipMemcpyAsync(out_codes, h->ap_codes.p, n * M, out, h->stream));
    if (out_norm_codes)
        HIP_TRY(hipMemcpyAsync(out_norm_codes, h->ap_ncodes.p, n, out, h->stream));
    if (out_idx)
        HIP_TRY(hipMemcpyAsync(out_idx, sidx, n * sizeof(uint32_t), out, h->stream));
    if (n_removed)
        return upsert_core(h, n, sidx, h->ap_ids.as<uint32_t>(), h->ap_codes.as<uint8_t>(), h->ap_ncodes.as<uint8_t>(), n_removed,
                           nullptr);
    return append_core(h, n, sidx, h->ap_ids.as<uint32_t>(), h->ap_codes.as<uint8_t>(), h->ap_ncodes.as<uint8_t>());
}

int ivfhnsw_gpu_add(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *precomputed_idx, size_t efSearch,
                    const uint32_t *ids, uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes)
{
    return add_impl(h, n, x, precomputed_idx, efSearch, ids, out_idx, out_codes, out_norm_codes, false, "add");
}

int ivfhnsw_gpu_add_dev(ivfhnsw_gpu *h, size_t n, const float *d_x, const uint32_t *d_precomputed_idx, size_t efSearch,
                        const uint32_t *d_ids, uint32_t *d_out_idx, uint8_t *d_out_codes, uint8_t *d_out_norm_codes)
{
    return add_impl(h, n, d_x, d_precomputed_idx, efSearch, d_ids, d_out_idx, d_out_codes, d_out_norm_codes, true, "add_dev");
}

// ---------------------------------------------------------------------------------------------------------------
// additions to a Grouping index: codes at the ends of sub-groups, and whole groups into empty lists
static int grouping_append_state(ivfhnsw_gpu *h, const char *who)
{
    int rc = table_change_guard(h, kAppends, who, true);
    if (rc)
        return rc;
    if (!h->has_group)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle holds no grouping tables (IVFADC lists grow by append_ivf)", who);
    return IVFHNSW_OK;
}

// the table rows add_groups installs with its codes: ga_cidx / ga_off / ga_nn / ga_alpha hold them, inter null = computed
struct GroupRows {
    size_t ngroups;
    const float *d_inter;
};

// d_list / d_sub [n] (checked here, on the device, before anything changes), d_ids [n], d_codes [n][M] (dword aligned),
// d_ncodes [n]: device memory, read on the handle's stream.  rows: the groups whose table rows go in with the batch (n may
// be 0 then).  Returns with the stream drained.  Bad ids and every device allocation (the dedupe sample's included) come
// before the first table row is written, so those errors leave the handle's tables the ones it had; behind that point
// only a failing launch or copy (a lost device) can stop the call.
static int grouping_append_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list, const uint32_t *d_sub,
                                const uint32_t *d_ids, const uint8_t *d_codes, const uint8_t *d_ncodes, const GroupRows *rows)
try {
    const size_t nc = h->t.nc, nsubc = (size_t)h->g.nsubc, nsub = nc * nsubc;
    int rc;
    auto write_rows = [&]() -> hipError_t {
        if (!rows)
            return hipSuccess;
        return launch_groups_rows(h->stream, h->ga_cidx.as<uint32_t>(), h->ga_off.as<unsigned long long>(),
                                  h->ga_nn.as<uint32_t>(), h->ga_alpha.as<float>(), rows->d_inter, h->gr.vectors, h->t.d,
                                  (uint32_t)nsubc, rows->ngroups, h->g_nn.as<uint32_t>(), h->g_alpha.as<float>(),
                                  h->g_inter.as<float>());
    };
    int dedupe = h->g.dedupe;
    if ((rc = grouping_dedupe_reserve(h)))
        return rc;
    if (n == 0) { // neighbour rows of empty groups only
        HIP_TRY(write_rows());
        if ((rc = grouping_dedupe_dev(h, h->g.sub_sizes, h->g.nn_idx, &dedupe)))
            return rc;
        h->g.dedupe = dedupe;
        return IVFHNSW_OK;
    }
    if ((rc = h->gp_sizes.ensure(nsub * sizeof(uint32_t))))
        return rc;
    uint32_t *sizes2 = h->gp_sizes.as<uint32_t>();
    bool bad_id = false;
    uint64_t n_local2 = 0;
    if ((rc = append_count(h, n, d_list, d_sub, sizes2, &bad_id, &n_local2)))
        return rc;
    if (bad_id)
        return fail(IVFHNSW_ERR_INVALID, "append_grouping: a list id is >= nc = %zu or a sub-group id >= nsubc = %zu", nc, nsubc);
    if ((rc = append_workspace(h, n, n_local2)) || (rc = h->gp_pre_old.ensure(nsub * sizeof(uint32_t))) ||
        (rc = h->gp_pre_new.ensure(nsub * sizeof(uint32_t))))
        return rc;
    // the new arrays first: the old ones stay the handle's until the new ones are complete
    ListArrays fresh;
    if ((rc = fresh.allocate(nc, n_local2, h->t.M)))
        return rc;
    const NewLists nl = fresh.view(n_local2);
    // stable order by (list, sub-group): by sub-group first, then from that order by list
    uint32_t *perm = nullptr, *tiles = h->ap_tiles.as<uint32_t>();
    const uint32_t *nstart = h->ap_cnt.as<uint32_t>(), *lstart = h->ap_own.as<uint32_t>(); // scanned in place by launch_append_tables
    uint32_t *pa = h->ap_perm.as<uint32_t>(), *pb = h->ap_perm2.as<uint32_t>(), *hist = h->ap_hist.as<uint32_t>();
    const SubGroups sg{(uint32_t)nsubc, d_sub, h->g.sub_sizes, h->gp_pre_old.as<uint32_t>(), h->gp_pre_new.as<uint32_t>()};
    hipError_t e = write_rows();
    if (e == hipSuccess)
        e = launch_sort_by_key(h->stream, d_sub, n, bits_of(nsubc - 1), pa, pb, hist, &perm);
    if (e == hipSuccess)
        e = launch_sort_by_key_from(h->stream, d_list, n, bits_of(nc - 1), perm, pa, pb, hist, &perm);
    if (e == hipSuccess)
        e = launch_append_layout(h->stream, h->t, nstart, lstart, tiles, nl);
    if (e == hipSuccess)
        e = launch_grouping_prefix(h->stream, nstart, sg.sizes, sizes2, h->gp_pre_old.as<uint32_t>(),
                                   h->gp_pre_new.as<uint32_t>(), (uint32_t)nc, sg.nsubc);
    if (e == hipSuccess)
        e = launch_append_merge(h->stream, h->t, nstart, lstart, tiles, &sg, nl);
    if (e == hipSuccess)
        e = launch_append_scatter(h->stream, h->t, perm, d_list, n, nstart, lstart, &sg, d_codes, d_ncodes, d_ids, nl);
    return commit_lists(h, "append_grouping", e, fresh, n_local2, &h->gp_sizes);
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "append_grouping: host allocation failed");
}

int ivfhnsw_gpu_append_grouping(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *sub_idx,
                                const uint32_t *ids, const uint8_t *codes, const uint8_t *norm_codes)
{
    int rc = grouping_append_state(h, "append_grouping");
    if (rc || n == 0)
        return rc;
    if (!list_idx || !sub_idx || !ids || !codes || !norm_codes)
        return fail(IVFHNSW_ERR_INVALID, "append_grouping: null buffer");
    if ((rc = append_size(h, n, "append_grouping")))
        return rc;
    for (size_t i = 0; i < n; i++)
        if (list_idx[i] >= h->t.nc || sub_idx[i] >= (uint32_t)h->g.nsubc)
            return fail(IVFHNSW_ERR_INVALID, "append_grouping: (list_idx, sub_idx)[%zu] = (%u, %u), nc = %u, nsubc = %d", i,
                        list_idx[i], sub_idx[i], h->t.nc, h->g.nsubc);
    if ((rc = stage_batch(h, n, list_idx, sub_idx, ids, codes, norm_codes)))
        return rc;
    return grouping_append_core(h, n, h->ap_idx.as<uint32_t>(), h->gp_sub.as<uint32_t>(), h->ap_ids.as<uint32_t>(),
                                h->ap_codes.as<uint8_t>(), h->ap_ncodes.as<uint8_t>(), nullptr);
}

int ivfhnsw_gpu_append_grouping_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list_idx, const uint32_t *d_sub_idx,
                                    const uint32_t *d_ids, const uint8_t *d_codes, const uint8_t *d_norm_codes)
{
    int rc = grouping_append_state(h, "append_grouping_dev");
    if (rc || n == 0)
        return rc;
    if (!d_list_idx || !d_sub_idx || !d_ids || !d_codes || !d_norm_codes)
        return fail(IVFHNSW_ERR_INVALID, "append_grouping_dev: null buffer");
    if (((uintptr_t)d_list_idx | (uintptr_t)d_sub_idx | (uintptr_t)d_ids | (uintptr_t)d_codes) & 3)
        return fail(IVFHNSW_ERR_INVALID, "append_grouping_dev: list_idx, sub_idx, ids and codes must be 4-byte aligned");
    if ((rc = append_size(h, n, "append_grouping_dev")))
        return rc;
    return grouping_append_core(h, n, d_list_idx, d_sub_idx, d_ids, d_codes, d_norm_codes, nullptr);
}

// encode_groups into the staging, the checks that need the handle's lists, then one append with the groups' table rows
static int add_groups_impl(ivfhnsw_gpu *h, size_t ngroups, const uint32_t *centroid_idx_in, const uint64_t *offsets_in,
                           const float *x, size_t efSearch, const uint32_t *ids, const float *inter, uint32_t *out_nn,
                           float *out_alphas, uint32_t *out_sub, uint8_t *out_codes, uint8_t *out_norm_codes, bool dev,
                           const char *who)
try {
    int rc = grouping_append_state(h, who);
    if (rc || (rc = check_add_ready(h, who)))
        return rc;
    if (ngroups == 0)
        return IVFHNSW_OK;
    if (!centroid_idx_in || !offsets_in || !out_nn || !out_alphas)
        return fail(IVFHNSW_ERR_INVALID, "%s: null buffer", who);
    const size_t nc = h->t.nc, nsubc = (size_t)h->g.nsubc;
    // the groups' ids and point offsets steer the chunking on the host: the _dev form brings them over first
    std::vector<uint32_t> cidx_h;
    std::vector<uint64_t> off_h;
    const uint32_t *centroid_idx = centroid_idx_in;
    const uint64_t *offsets = offsets_in;
    if (dev) {
        if (((uintptr_t)centroid_idx_in | (uintptr_t)x | (uintptr_t)ids | (uintptr_t)inter | (uintptr_t)out_nn |
             (uintptr_t)out_alphas | (uintptr_t)out_sub | (uintptr_t)out_codes) & 3 || (uintptr_t)offsets_in & 7)
            return fail(IVFHNSW_ERR_INVALID, "%s: device pointers must be 4-byte aligned (offsets 8-byte)", who);
        cidx_h.resize(ngroups);
        off_h.resize(ngroups + 1);
        HIP_TRY(hipStreamSynchronize(h->stream));
        HIP_TRY(hipMemcpy(cidx_h.data(), centroid_idx_in, ngroups * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIP_TRY(hipMemcpy(off_h.data(), offsets_in, (ngroups + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        centroid_idx = cidx_h.data();
        offsets = off_h.data();
    }
    if (offsets[0] != 0)
        return fail(IVFHNSW_ERR_INVALID, "%s: offsets[0] must be 0", who);
    for (size_t g = 0; g < ngroups; g++) {
        if (offsets[g + 1] < offsets[g])
            return fail(IVFHNSW_ERR_INVALID, "%s: offsets not monotone at group %zu", who, g);
        if (centroid_idx[g] >= nc)
            return fail(IVFHNSW_ERR_INVALID, "%s: centroid_idx[%zu] = %u, nc = %zu", who, g, centroid_idx[g], nc);
    }
    {
        std::vector<uint32_t> sorted(centroid_idx, centroid_idx + ngroups);
        std::sort(sorted.begin(), sorted.end());
        const auto dup = std::adjacent_find(sorted.begin(), sorted.end());
        if (dup != sorted.end())
            return fail(IVFHNSW_ERR_INVALID, "%s: centroid %u appears twice in one call", who, *dup);
    }
    const size_t n = offsets[ngroups];
    if (n && (!ids || !x))
        return fail(IVFHNSW_ERR_INVALID, "%s: null buffer", who);
    if ((rc = append_size(h, n, who)))
        return rc;
    if ((rc = h->ga_cidx.ensure(ngroups * sizeof(uint32_t))) || (rc = h->ga_off.ensure((ngroups + 1) * sizeof(uint64_t))) ||
        (rc = h->ga_nn.ensure(ngroups * nsubc * sizeof(uint32_t))) || (rc = h->ga_alpha.ensure(ngroups * sizeof(float))) ||
        (rc = h->ga_status.ensure(sizeof(uint32_t))) || (rc = append_stage(h, n)) || (rc = h->gp_sub.ensure(n * sizeof(uint32_t))) ||
        (inter && !dev && (rc = h->ga_inter.ensure(ngroups * nsubc * sizeof(float)))))
        return rc;
    HIP_TRY(hipMemcpyAsync(h->ga_cidx.p, centroid_idx, ngroups * sizeof(uint32_t), hipMemcpyHostToDevice, h->stream));
    HIP_TRY(hipMemcpyAsync(h->ga_off.p, offsets, (ngroups + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, h->stream));
    // a group that holds codes cannot be added to: its alpha and neighbours would be overwritten under them
    uint32_t first = 0xffffffffu;
    if ((rc = run_with_word(h, h->ga_status, 0xff, [&](uint32_t *status) {
             return launch_groups_empty(h->stream, h->t.goff, h->ga_cidx.as<uint32_t>(), ngroups, (uint32_t)nc, status);
         }, &first)))
        return rc;
    if (first != 0xffffffffu)
        return fail(IVFHNSW_ERR_STATE, "%s: list %u (group %u of the call) already holds codes; a second add_group on a "
                    "centroid has no counterpart in a search (remove its ids first)", who, centroid_idx[first], first);
    const float *d_inter = nullptr;
    if (inter && dev) {
        d_inter = inter;
    } else if (inter) {
        HIP_TRY(hipMemcpyAsync(h->ga_inter.p, inter, ngroups * nsubc * sizeof(float), hipMemcpyHostToDevice, h->stream));
        d_inter = h->ga_inter.as<float>();
    }
    if ((rc = encode_groups_impl(h, ngroups, nsubc, centroid_idx, offsets, x, efSearch, out_nn, out_alphas, out_sub, out_codes,
                                 out_norm_codes, dev, true)))
        return rc;
    if (n)
        HIP_TRY(hipMemcpyAsync(h->ap_ids.p, ids, n * sizeof(uint32_t), dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                               h->stream));
    const GroupRows rows{ngroups, d_inter};
    return grouping_append_core(h, n, h->ap_idx.as<uint32_t>(), h->gp_sub.as<uint32_t>(), h->ap_ids.as<uint32_t>(),
                                h->ap_codes.as<uint8_t>(), h->ap_ncodes.as<uint8_t>(), &rows);
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "%s: host allocation failed", who);
}

int ivfhnsw_gpu_add_groups(ivfhnsw_gpu *h, size_t ngroups, const uint32_t *centroid_idx, const uint64_t *offsets, const float *x,
                           size_t efSearch, const uint32_t *ids, const float *inter_centroid_dists,
                           uint32_t *out_nn_centroid_idxs, float *out_alphas, uint32_t *out_subcentroid_idxs, uint8_t *out_codes,
                           uint8_t *out_norm_codes)
{
    return add_groups_impl(h, ngroups, centroid_idx, offsets, x, efSearch, ids, inter_centroid_dists, out_nn_centroid_idxs,
                           out_alphas, out_subcentroid_idxs, out_codes, out_norm_codes, false, "add_groups");
}

int ivfhnsw_gpu_add_groups_dev(ivfhnsw_gpu *h, size_t ngroups, const uint32_t *d_centroid_idx, const uint64_t *d_offsets,
                               const float *d_x, size_t efSearch, const uint32_t *d_ids, const float *d_inter_centroid_dists,
                               uint32_t *d_out_nn_centroid_idxs, float *d_out_alphas, uint32_t *d_out_subcentroid_idxs,
                               uint8_t *d_out_codes, uint8_t *d_out_norm_codes)
{
    return add_groups_impl(h, ngroups, d_centroid_idx, d_offsets, d_x, efSearch, d_ids, d_inter_centroid_dists,
                           d_out_nn_centroid_idxs, d_out_alphas, d_out_subcentroid_idxs, d_out_codes, d_out_norm_codes, true,
                           "add_groups_dev");
}

// ---------------------------------------------------------------------------------------------------------------
// removals by label: a stable compaction of the lists into fresh arrays, swapped in when complete
static int remove_state(ivfhnsw_gpu *h, const char *who)
{
    int rc = table_change_guard(h, kRemovals, who, true);
    if (rc)
        return rc;
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle is shard %u of %u; a shard cannot update the global offsets of the "
                    "lists other shards own, so sharded handles have no removal", who, h->t.shard_rank, h->t.shard_world);
    return IVFHNSW_OK;
}

// d_labels [n] (device memory, n > 0, max_label = their maximum), read on the handle's stream.  rem_out [nc] (device,
// nullable) receives the codes removed per list.  Returns with the stream drained; on any error the handle's tables are
// the ones it had.  Nothing removed: no table is reallocated.
static int remove_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint32_t max_label, uint64_t *n_removed,
                       uint32_t *rem_out)
try {
    const size_t nc = h->t.nc, len = nc + 1;
    const uint64_t n_local = h->n_local;
    const size_t ntiles = update_tiles(n_local, kRemoveTileRows);
    const bool grp = h->has_group;
    const size_t nsub = grp ? nc * (size_t)h->g.nsubc : 0;
    int rc;
    if ((rc = h->rm_mask.ensure(remove_mask_words(ntiles, kRemoveTileRows) * sizeof(uint64_t))) ||
        (rc = h->rm_keep.ensure((ntiles + 1) * sizeof(uint32_t))) || (rc = h->rm_rem.ensure(len * sizeof(uint32_t))) ||
        (rc = h->rm_part.ensure(append_scan_parts(std::max(len, ntiles + 1)) * sizeof(uint32_t))) ||
        (rc = h->rm_sizes.ensure(nsub * sizeof(uint32_t))))
        return rc;
    uint32_t *keep = h->rm_keep.as<uint32_t>(), *rem = h->rm_rem.as<uint32_t>(), *part = h->rm_part.as<uint32_t>();
    unsigned long long *mask = h->rm_mask.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(keep + ntiles, 0, sizeof(uint32_t), h->stream));
    if ((rc = labels_bitmap(h, n, d_labels, max_label, h->rm_bits)))
        return rc;
    HIP_TRY(launch_remove_mark(h->stream, h->t, n_local, h->rm_bits.as<uint32_t>(), max_label, mask, keep));
    HIP_TRY(launch_remove_counts(h->stream, h->t, mask, grp ? h->g.sub_sizes : nullptr, h->rm_sizes.as<uint32_t>(),
                                 grp ? h->g.nsubc : 0, rem, rem_out));
    HIP_TRY(launch_scan_excl_u32(h->stream, rem, len, part));
    HIP_TRY(launch_scan_excl_u32(h->stream, keep, ntiles + 1, part));
    uint32_t removed = 0, kept = 0;
    HIP_TRY(hipMemcpyAsync(&removed, rem + nc, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&kept, keep + ntiles, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((uint64_t)removed + kept != n_local)
        return fail(IVFHNSW_ERR_HIP, "remove_ids: %u removed + %u kept != %llu codes", removed, kept,
                    (unsigned long long)n_local);
    *n_removed = removed;
    if (removed == 0)
        return IVFHNSW_OK;
    const uint64_t n_local2 = kept;
    // the new arrays first: the old ones stay the handle's until the new ones are complete.  The dedupe sample's
    // workspace too, so that nothing is allocated behind the compaction
    ListArrays fresh;
    if ((rc = fresh.allocate(nc, n_local2, h->t.M)) || (grp && (rc = grouping_dedupe_reserve(h))))
        return rc;
    const hipError_t e = launch_remove_compact(h->stream, h->t, n_local, mask, rem, keep, fresh.view(n_local2));
    return commit_lists(h, "remove_ids", e, fresh, n_local2, grp ? &h->rm_sizes : nullptr);
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "remove_ids: host allocation failed");
}

int ivfhnsw_gpu_remove_ids(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, uint64_t *n_removed, uint32_t *removed_per_list)
{
    int rc = remove_state(h, "remove_ids");
    if (rc)
        return rc;
    if ((rc = label_args_guard(n, labels, "remove_ids")))
        return rc;
    if (n_removed)
        *n_removed = 0;
    if (removed_per_list)
        memset(removed_per_list, 0, (size_t)h->t.nc * sizeof(uint32_t));
    if (n == 0 || h->n_local == 0)
        return IVFHNSW_OK;
    uint32_t mx = 0;
    if ((removed_per_list && (rc = h->rm_out.ensure((size_t)h->t.nc * sizeof(uint32_t)))) ||
        (rc = labels_from_host(h, n, labels, h->rm_labels, &mx)))
        return rc;
    uint64_t removed = 0;
    if ((rc = remove_core(h, n, h->rm_labels.as<uint32_t>(), mx, &removed, removed_per_list ? h->rm_out.as<uint32_t>() : nullptr)))
        return rc;
    if (removed_per_list && removed)
        HIP_TRY(hipMemcpy(removed_per_list, h->rm_out.p, (size_t)h->t.nc * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_removed)
        *n_removed = removed;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_remove_ids_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint64_t *n_removed,
                               uint32_t *d_removed_per_list)
{
    int rc = remove_state(h, "remove_ids_dev");
    if (rc)
        return rc;
    if ((rc = label_args_guard(n, d_labels, "remove_ids_dev")))
        return rc;
    if (n_removed)
        *n_removed = 0;
    if (n == 0 || h->n_local == 0) {
        if (d_removed_per_list) {
            HIP_TRY(hipMemsetAsync(d_removed_per_list, 0, (size_t)h->t.nc * sizeof(uint32_t), h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        return IVFHNSW_OK;
    }
    uint32_t mx = 0;
    if ((rc = labels_max_dev(h, h->rm_status, n, d_labels, &mx)))
        return rc;
    uint64_t removed = 0;
    if ((rc = remove_core(h, n, d_labels, mx, &removed, d_removed_per_list)))
        return rc;
    if (n_removed)
        *n_removed = removed;
    return IVFHNSW_OK;
}

// ---------------------------------------------------------------------------------------------------------------
// upserts: the codes that bear one of the batch's labels leave and the batch's codes go to the ends of
// their lists, as remove_ids followed by append_ivf would leave them -- in one rebuild and one commit
static int upsert_state(ivfhnsw_gpu *h, const char *who)
{
    int rc = append_state(h, who);
    if (rc)
        return rc;
    if (h->t.shard_world > 1)
        return fail(IVFHNSW_ERR_STATE, "%s: the handle is shard %u of %u; sharded handles have no removal, so no upsert", who,
                    h->t.shard_rank, h->t.shard_world);
    return IVFHNSW_OK;
}

// d_idx [n] and d_ids [n] (both checked here, on the device, before anything changes: every list id < nc, no label twice),
// d_codes [n][M] (dword aligned), d_ncodes [n]: device memory, n > 0, read on the handle's stream.  rem_out [nc] (device,
// nullable) receives the codes removed per list.  Returns with the stream drained; on any error the handle's tables are
// the ones it had.  The steps are removal's (mask, keep, rem) and append's (cnt, the sort); the layout and the two copies
// are kernels_upsert.hip's.
static int upsert_core(ivfhnsw_gpu *h, size_t n, const uint32_t *d_idx, const uint32_t *d_ids, const uint8_t *d_codes,
                       const uint8_t *d_ncodes, uint64_t *n_removed, uint32_t *rem_out)
try {
    const size_t nc = h->t.nc, len = nc + 1;
    const uint64_t n_local = h->n_local;
    const size_t ntiles = update_tiles(n_local, kRemoveTileRows);
    int rc;
    bool bad_id = false;
    uint64_t grown = 0;
    if ((rc = append_count(h, n, d_idx, nullptr, nullptr, &bad_id, &grown)))
        return rc;
    if (bad_id)
        return fail(IVFHNSW_ERR_INVALID, "upsert: a list id is >= nc = %zu", nc);
    uint32_t max_label = 0, twice = 0;
    if ((rc = labels_max_dev(h, h->rm_status, n, d_ids, &max_label)) ||
        (rc = h->rm_bits.ensure(label_bitmap_words(max_label) * sizeof(uint32_t))) ||
        (rc = run_with_word(h, h->rm_status, 0, [&](uint32_t *status) {
             return launch_upsert_bits(h->stream, d_ids, n, max_label, h->rm_bits.as<uint32_t>(), status);
         }, &twice)))
        return rc;
    if (twice)
        return fail(IVFHNSW_ERR_INVALID, "upsert: a label comes twice in one batch (after an upsert one row bears each label)");
    if ((rc = h->rm_mask.ensure(remove_mask_words(ntiles, kRemoveTileRows) * sizeof(uint64_t))) ||
        (rc = h->rm_keep.ensure((ntiles + 1) * sizeof(uint32_t))) || (rc = h->rm_rem.ensure(len * sizeof(uint32_t))) ||
        (rc = h->rm_part.ensure(append_scan_parts(std::max(len, ntiles + 1)) * sizeof(uint32_t))))
        return rc;
    uint32_t *keep = h->rm_keep.as<uint32_t>(), *rem = h->rm_rem.as<uint32_t>(), *part = h->rm_part.as<uint32_t>();
    unsigned long long *mask = h->rm_mask.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(keep + ntiles, 0, sizeof(uint32_t), h->stream));
    HIP_TRY(launch_remove_mark(h->stream, h->t, n_local, h->rm_bits.as<uint32_t>(), max_label, mask, keep));
    HIP_TRY(launch_remove_counts(h->stream, h->t, mask, nullptr, nullptr, 0, rem, rem_out));
    HIP_TRY(launch_scan_excl_u32(h->stream, rem, len, part));
    HIP_TRY(launch_scan_excl_u32(h->stream, keep, ntiles + 1, part));
    uint32_t removed = 0, kept = 0;
    HIP_TRY(hipMemcpyAsync(&removed, rem + nc, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipMemcpyAsync(&kept, keep + ntiles, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIP_TRY(hipStreamSynchronize(h->stream));
    if ((uint64_t)removed + kept != n_local || grown != n_local + n)
        return fail(IVFHNSW_ERR_HIP, "upsert: %u removed + %u kept != %llu codes, or %llu != %llu + %zu", removed, kept,
                    (unsigned long long)n_local, (unsigned long long)grown, (unsigned long long)n_local, n);
    const uint64_t n_local2 = (uint64_t)kept + n;
    const size_t nblocks = (n + kKmeansTile - 1) / kKmeansTile;
    if ((rc = h->ap_perm.ensure(n * sizeof(uint32_t))) || (rc = h->ap_perm2.ensure(n * sizeof(uint32_t))) ||
        (rc = h->ap_hist.ensure(256 * nblocks * sizeof(uint32_t))) || (rc = h->ap_tiles.ensure((ntiles + 1) * sizeof(uint32_t))))
        return rc;
    // the new arrays, one set: the old ones stay the handle's until the new ones are complete
    ListArrays fresh;
    if ((rc = fresh.allocate(nc, n_local2, h->t.M)))
        return rc;
    const NewLists nl = fresh.view(n_local2);
    uint32_t *perm = nullptr, *tiles = h->ap_tiles.as<uint32_t>();
    const uint32_t *nstart = h->ap_cnt.as<uint32_t>(); // scanned in place by launch_append_tables
    hipError_t e = launch_sort_by_key(h->stream, d_idx, n, bits_of(nc - 1), h->ap_perm.as<uint32_t>(), h->ap_perm2.as<uint32_t>(),
                                      h->ap_hist.as<uint32_t>(), &perm);
    if (e == hipSuccess)
        e = launch_upsert_layout(h->stream, h->t, n_local, rem, nstart, tiles, nl);
    if (e == hipSuccess)
        e = launch_upsert_compact(h->stream, h->t, n_local, mask, keep, nstart, tiles, nl);
    if (e == hipSuccess)
        e = launch_upsert_scatter(h->stream, h->t, perm, d_idx, n, nstart, rem, d_codes, d_ncodes, d_ids, nl);
    if ((rc = commit_lists(h, "upsert", e, fresh, n_local2, nullptr)))
        return rc;
    h->last_nq = 0; // the last search's plan and candidate stream described the old rows
    h->last_stream = false;
    *n_removed = removed;
    return IVFHNSW_OK;
} catch (const std::bad_alloc &) {
    return fail(IVFHNSW_ERR_NOMEM, "upsert: host allocation failed");
}

int ivfhnsw_gpu_upsert_ivf(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *ids, const uint8_t *codes,
                           const uint8_t *norm_codes, uint64_t *n_removed, uint32_t *removed_per_list)
{
    int rc = upsert_state(h, "upsert_ivf");
    if (rc)
        return rc;
    if (n && (!list_idx || !ids || !codes || !norm_codes))
        return fail(IVFHNSW_ERR_INVALID, "upsert_ivf: null buffer");
    if (n && (rc = append_size(h, n, "upsert_ivf")))
        return rc;
    for (size_t i = 0; i < n; i++)
        if (list_idx[i] >= h->t.nc)
            return fail(IVFHNSW_ERR_INVALID, "upsert_ivf: list_idx[%zu] = %u, nc = %u", i, list_idx[i], h->t.nc);
    if (n_removed)
        *n_removed = 0;
    if (removed_per_list)
        memset(removed_per_list, 0, (size_t)h->t.nc * sizeof(uint32_t));
    if (n == 0)
        return IVFHNSW_OK;
    if ((removed_per_list && (rc = h->rm_out.ensure((size_t)h->t.nc * sizeof(uint32_t)))) ||
        (rc = stage_batch(h, n, list_idx, nullptr, ids, codes, norm_codes)))
        return rc;
    uint64_t removed = 0;
    if ((rc = upsert_core(h, n, h->ap_idx.as<uint32_t>(), h->ap_ids.as<uint32_t>(), h->ap_codes.as<uint8_t>(),
                          h->ap_ncodes.as<uint8_t>(), &removed, removed_per_list ? h->rm_out.as<uint32_t>() : nullptr)))
        return rc;
    if (removed_per_list)
        HIP_TRY(hipMemcpy(removed_per_list, h->rm_out.p, (size_t)h->t.nc * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (n_removed)
        *n_removed = removed;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_upsert_ivf_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list_idx, const uint32_t *d_ids, const uint8_t *d_codes,
                               const uint8_t *d_norm_codes, uint64_t *n_removed, uint32_t *d_removed_per_list)
{
    int rc = upsert_state(h, "upsert_ivf_dev");
    if (rc)
        return rc;
    if (n && (!d_list_idx || !d_ids || !d_codes || !d_norm_codes))
        return fail(IVFHNSW_ERR_INVALID, "upsert_ivf_dev: null buffer");
    if (((uintptr_t)d_list_idx | (uintptr_t)d_ids | (uintptr_t)d_codes | (uintptr_t)d_removed_per_list) & 3)
        return fail(IVFHNSW_ERR_INVALID, "upsert_ivf_dev: list_idx, ids, codes and removed_per_list must be 4-byte aligned");
    if (n && (rc = append_size(h, n, "upsert_ivf_dev")))
        return rc;
    if (n_removed)
        *n_removed = 0;
    if (n == 0) {
        if (d_removed_per_list) {
            HIP_TRY(hipMemsetAsync(d_removed_per_list, 0, (size_t)h->t.nc * sizeof(uint32_t), h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
        }
        return IVFHNSW_OK;
    }
    uint64_t removed = 0;
    if ((rc = upsert_core(h, n, d_list_idx, d_ids, d_codes, d_norm_codes, &removed, d_removed_per_list)))
        return rc;
    if (n_removed)
        *n_removed = removed;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_upsert(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *precomputed_idx, size_t efSearch,
                       const uint32_t *ids, uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes, uint64_t *n_removed)
{
    uint64_t removed = 0;
    const int rc = add_impl(h, n, x, precomputed_idx, efSearch, ids, out_idx, out_codes, out_norm_codes, false, "upsert", &removed);
    if (n_removed)
        *n_removed = rc ? 0 : removed;
    return rc;
}

int ivfhnsw_gpu_upsert_dev(ivfhnsw_gpu *h, size_t n, const float *d_x, const uint32_t *d_precomputed_idx, size_t efSearch,
                           const uint32_t *d_ids, uint32_t *d_out_idx, uint8_t *d_out_codes, uint8_t *d_out_norm_codes,
                           uint64_t *n_removed)
{
    uint64_t removed = 0;
    const int rc = add_impl(h, n, d_x, d_precomputed_idx, efSearch, d_ids, d_out_idx, d_out_codes, d_out_norm_codes, true,
                            "upsert_dev", &removed);
    if (n_removed)
        *n_removed = rc ? 0 : removed;
    return rc;
}
