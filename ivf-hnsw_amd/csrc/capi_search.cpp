// The batched search pipeline (rotate -> coarse -> table -> plan -> scan -> select) and its host-pointer entry points.
#include "capi_internal.h"
#include "walk_form.h"

// a size from the environment, def when unset or empty; every caller reads its knob once per process
static size_t env_size(const char *name, size_t def)
{
    const char *e = getenv(name);
    return (e && *e) ? (size_t)atol(e) : def;
}

// what ivfhnsw_gpu_search, ivfhnsw_gpu_search_keys and every chunk of search_dev check first, behind bind
int ivfhnsw_gpu_impl::search_args_guard(const ivfhnsw_gpu *h, const ivfhnsw_search_params *p, size_t k)
{
    if (!h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "search before upload_ivf");
    if (!p || p->nprobe == 0 || k == 0)
        return fail(IVFHNSW_ERR_INVALID, "nprobe and k must be positive");
    return IVFHNSW_OK;
}

// The host-pointer entry points: a staging buffer of `bytes` filled from host memory, and one copied back to it, on the
// handle's stream.
int ivfhnsw_gpu_impl::stage_in(ivfhnsw_gpu *h, DevBuf &b, const void *src, size_t bytes)
{
    int rc = b.ensure(bytes);
    if (rc)
        return rc;
    HIP_TRY(hipMemcpyAsync(b.p, src, bytes, hipMemcpyHostToDevice, h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_impl::stage_out(ivfhnsw_gpu *h, void *dst, const DevBuf &b, size_t bytes)
{
    HIP_TRY(hipMemcpyAsync(dst, b.p, bytes, hipMemcpyDeviceToHost, h->stream));
    return IVFHNSW_OK;
}

// Scratch of the walk (h->walk) for nslots queries in flight, `words` of bitmap each: first half the visited bitmaps
// (the LDS set's overflow store), second half the tail bitmaps of the redo form (walk_set.h TailSpill) -- always at the
// middle of the ALLOCATION, so that no launch's visited area ever overlaps them; both halves zero between launches
static int walk_scratch(ivfhnsw_gpu *h, size_t words, size_t nslots, size_t nq, uint32_t **tails)
{
    int rc = h->w_visited.ensure(words * sizeof(uint32_t) * std::max<size_t>(nslots, 64) * 2);
    if (rc)
        return rc;
    if (h->w_visited.p != h->walk.zero_ptr || h->w_visited.bytes != h->walk.zero_bytes) {
        HIP_TRY(hipMemsetAsync(h->w_visited.p, 0, h->w_visited.bytes, h->stream)); // (re)allocated: contents unknown
        h->walk.zero = true;
        h->walk.zero_ptr = h->w_visited.p;
        h->walk.zero_bytes = h->w_visited.bytes;
    }
    *tails = reinterpret_cast<uint32_t *>(h->w_visited.as<char>() + h->w_visited.bytes / 2);
    return h->w_redo.ensure(nq * sizeof(uint32_t));
}

static int coarse_dev_impl(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t nprobe, size_t efSearch,
                           uint32_t *d_coarse_ids, float *d_coarse_dists, const SearchCall &call, WalkClear &meet)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "coarse search needs upload_quantizer");
    if (nprobe == 0 || efSearch < nprobe)
        return fail(IVFHNSW_ERR_INVALID, "efSearch %zu < nprobe %zu (precondition of IndexIVF_HNSW.cpp:249-258)",
                    efSearch, nprobe);
    if (efSearch > 1024)
        return fail(IVFHNSW_ERR_INVALID, "efSearch %zu > 1024 unsupported on the device", efSearch);
    if (nq == 0)
        return IVFHNSW_OK;
    if (nq > 0x7fffffffull)
        return fail(IVFHNSW_ERR_INVALID, "nq too large");
    // one visited bitmap per query in flight
    const size_t words = ((((size_t)h->gr.n + 31) / 32) + 3) & ~(size_t)3;
    StageScope sc(h, IVFHNSW_STAGE_COARSE);
    // few queries (the reference's drivers: one per call): a workgroup per query on the fat graph, when it was prepared
    static const size_t lat_max_nq = env_size("IVFHNSW_LATENCY_MAX_NQ", 256);
    StatusWords *st = status_words(h);
    uint32_t *tails = nullptr;
    if (!call.no_latency && nq <= lat_max_nq && coarse_latency_supported(h->gr, (int)efSearch)) {
        uint32_t *hdr = &st->redo_len;
        const bool defer = call.defer_redo; // the caller synchronises and reads the status word itself
        if (!defer) {
            if ((rc = walk_scratch(h, words, 64, nq, &tails)))
                return rc;
            HIP_TRY(hipMemsetAsync(hdr, 0, 3 * sizeof(uint32_t), h->stream)); // length, counter, exit count
        }
        HIP_TRY(launch_coarse_latency(h->stream, h->gr, d_queries, (int)nq, (int)nprobe, (int)efSearch, d_coarse_ids,
                                      d_coarse_dists, status_word(h), meet.keys, meet.done, defer ? nullptr : hdr,
                                      defer ? nullptr : h->w_redo.as<uint32_t>()));
        meet.cleared = meet.keys != nullptr;
        if (!defer)
            HIP_TRY(launch_coarse_redo(h->stream, h->gr, d_queries, (int)nq, (int)nprobe, (int)efSearch, d_coarse_ids,
                                       d_coarse_dists, h->w_visited.as<uint32_t>(), words, status_word(h), hdr,
                                       h->w_redo.as<uint32_t>(), tails, 64));
        return IVFHNSW_OK;
    }
    const int nslots = (int)std::min<size_t>(nq, (size_t)coarse_slots_for((int)efSearch));
    if ((rc = walk_scratch(h, words, (size_t)nslots, nq, &tails)))
        return rc;
    HIP_TRY(launch_coarse(h->stream, h->gr, d_queries, (int)nq, (int)nprobe, (int)efSearch, d_coarse_ids, d_coarse_dists,
                          h->w_visited.as<uint32_t>(), words, nslots, status_word(h), &st->walk_next,
                          h->w_visited.bytes / 2, &h->walk.zero, h->w_redo.as<uint32_t>(), tails, 64,
                          &h->walk.counters_clean));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_coarse_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t nprobe, size_t efSearch,
                           uint32_t *d_coarse_ids, float *d_coarse_dists)
{
    WalkClear meet;
    return coarse_dev_impl(h, nq, d_queries, nprobe, efSearch, d_coarse_ids, d_coarse_dists, SearchCall(), meet);
}

int ivfhnsw_gpu_rotate_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, float *d_out)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "rotate needs upload_ivf");
    if (nq == 0)
        return IVFHNSW_OK;
    if (!d_queries || !d_out || nq > 0x7fffffffull)
        return fail(IVFHNSW_ERR_INVALID, "null buffer or nq too large");
    if (h->t.opq_At) {
        StageScope sc(h, IVFHNSW_STAGE_OPQ);
        HIP_TRY(launch_opq(h->stream, h->t.opq_At, d_queries, d_out, (int)nq, h->t.d));
    } else if (d_out != d_queries) {
        HIP_TRY(hipMemcpyAsync(d_out, d_queries, nq * (size_t)h->t.d * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
    }
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_coarse(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t k, size_t efSearch, uint32_t *ids,
                       float *dists)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "coarse search needs upload_quantizer");
    if (nq == 0)
        return IVFHNSW_OK;
    if (!queries || !ids || !dists || k == 0)
        return fail(IVFHNSW_ERR_INVALID, "null buffer or k == 0");
    const size_t d = h->gr.d;
    if ((rc = h->s_cid.ensure(nq * k * sizeof(uint32_t))) || (rc = h->s_cd.ensure(nq * k * sizeof(float))) ||
        (rc = stage_in(h, h->s_q, queries, nq * d * sizeof(float))) ||
        (rc = ivfhnsw_gpu_coarse_dev(h, nq, h->s_q.as<float>(), k, efSearch, h->s_cid.as<uint32_t>(), h->s_cd.as<float>())) ||
        (rc = stage_out(h, ids, h->s_cid, nq * k * sizeof(uint32_t))) ||
        (rc = stage_out(h, dists, h->s_cd, nq * k * sizeof(float))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return check_status(h);
}

static int search_dev_chunk(ivfhnsw_gpu *h, const SearchArgs &a, SearchCall &call);

// one GPU, IVFADC: plan and tables are independent of each other and go in ONE launch (kernels_search.hip
// plan_lut_kernel; IVFHNSW_PLAN_LUT=0 keeps them apart) -- unless the table is left to the pipelined scan
static bool plan_lut_shape(const ivfhnsw_gpu *h)
{
    static const bool plan_lut_on = env_size("IVFHNSW_PLAN_LUT", 1) != 0;
    const int ds = h->t.dsub;
    return plan_lut_on && !h->has_group && h->t.shard_world == 1 && (ds == 4 || ds == 6 || ds == 8 || ds == 12 || ds == 16);
}

// One large batch as TWO uneven parts on two streams.  The walk's resident wavefronts pull queries from a counter, so a
// launch ends with a tail of partly idle CUs (10 000 queries on 4096 slots: 2.44 "rounds"), and the scan can only start
// when the last query has been walked.  Here the first ~78 % of the batch run on the handle's stream and the rest on an
// internal view (own workspace and stream, same tables): the second part's walk moves into the slots the first part's
// last round frees, and the first part's table + scan (LDS-bound) run beside it (HBM-bound).  Fork and join are events,
// so the call keeps its contract: everything is ordered behind the caller's stream and complete when that stream gets
// there.  Measured (tools/split_probe.py, 1B corpus, 10 k queries): 1.81 -> 1.67 ms per batch, the first part's scan at
// 4.8 instead of 5.0 TB/s; three parts give no more, four lose.  ON by default since round 3 (the first part's share by
// estimate, auto_split_permille; ivfhnsw_gpu_set_batch_split(h, 0) or IVFHNSW_SPLIT=0 = one part): a plain search_dev call should deliver the
// fastest exact form.  The price is in the scan's accounting: two launches per step, the first slowed a little by the walk
// beside it, the second a single round of workgroups -- 17 B x all codes over the summed launch time is 0.58-0.59 of the
// HBM peak where the one-launch form reads 0.62 (bench.py reports both).  Not for sharded calls (their resolve step
// needs one plan), heap-order k > 1 (one candidate stream), given coarse results (no walk to overlap) or batches below
// two rounds of the walk.
// Since round 4 a THIRD stream builds both parts' ADC tables while the walks run, where the second walk leaves resident
// slots for that (early_tables_wanted): each part's chain behind its walk is then redo, plan, scan.  Kernel trace of a step
// at (32, 10000, 80), before -> after, us from the first walk's start: walks end 1172 / 1486 -> 1210 / 1478, scans start
// 1252 / 1550 -> 1243 / 1518, chains end 1558 / 1635 -> 1542 / 1605; the table kernels ran from 22 to 1125 (first part, its
// workgroups entering as walk wavefronts leave) and 1132 to 1174 (second part).  The join covers the third stream through
// the chains: each waits for its tables in front of its scan.
static const size_t kSplitMinNq = 8192;

// The first part's share when nobody fixed it.  The second part's walk fills the tail of the first part's, the first part's
// table + plan + scan run beside the second part's walk, the second part's scan runs alone: the step is shortest where the
// second walk and the first scan take equally long, share = W / (W + S).  W and S per query from the call's own parameters,
// with rates measured at the 1B shapes on one MI355X: the walk 1.7 ns per unit of efSearch (1.37 / 1.63 /
// 2.56 ms per 10 k queries at 80 / 100 / 130), the scan (M + 1) bytes per code at 5 TB/s over the codes the max_codes rule
// lets through, the table 5 ns (nothing where it is built early, beside the walks), the Grouping plan ~90 ns and its scan
// at 0.8 of the rate.  Measured against fixed shares:
// (32, 10000, 80) 0.79 -> the 2048-query second part that measured best; (64, 30000, 100) 0.63 -> 4096, 3.97 -> 4.18 M
// queries/s; Grouping + pruning 0.49 -> 4096, 3.35 -> 3.44 M.  The estimate only has to land on the right multiple of 2048.
static int auto_split_permille(const ivfhnsw_gpu *h, const ivfhnsw_search_params *p, bool early_tables)
{
    const double walk = 1.7 * (double)p->efSearch;
    const double nc = (double)std::max<uint32_t>(h->t.nc, 1u);
    const double list = (double)h->n_local / nc;
    const double codes = std::min((double)p->nprobe * list, (double)p->max_codes + 0.5 * list);
    double scan = codes * (double)(h->t.M + 1) / 5000.0 + (early_tables ? 0.0 : 5.0); // early tables are on neither chain
    if (h->has_group)
        scan = scan / 0.8 + 90.0;
    const double share = walk / (walk + scan);
    return (int)std::min(900.0, std::max(400.0, share * 1000.0 + 0.5));
}

// Early tables (IVFHNSW_EARLY_LUT=0 = the launches of round 3): where a part would build plan and tables in one launch
// behind its walk (chunk_plan_table), the tables of BOTH parts are built on a third stream while the walks run.  lut_body
// reads only the (rotated) queries and the code book, and from the first walk's last round on resident slots stand empty:
// the 16 KB per query written there are off both chains, each of which then runs plan, scan.  Measured, alternating on one
// box (profiles/r04_early_tables.md): (32, 10000, 80) 1.652 -> 1.617 ms per step.  Only where the second part's walk leaves
// such slots, i.e. has fewer queries than the walk has resident wavefronts (search_dev_split): at (64, 30000, 100) its 4096
// queries take every slot the first walk frees, the table workgroups compete with them, and the step measured 0.6 %
// SLOWER (2.377 -> 2.390 ms; no other cut gained either).  Not for Grouping, shards, a filter, filter slots, tags, values or a table that the
// pipelined scan builds itself.
static bool early_tables_wanted(const ivfhnsw_gpu *h, const SearchArgs &a)
{
    static const bool on = env_size("IVFHNSW_EARLY_LUT", 1) != 0;
    if (!on || !plan_lut_shape(h) || h->filter.mode >= 0 || a.pick)
        return false;
    const bool may_pipe = a.k == 1 && h->opt_scan_pipe != 0 &&
                          scan_pipe_supported(h->t, (int)a.p->nprobe, (int)a.nq, 1, h->n_local > 0, h->opt_scan_pipe == 1);
    return !may_pipe;
}

// The helper stream and its events, once per handle.  The stream has the lowest priority, so that a walk's wavefronts win
// a freed slot ahead of table workgroups.  (The view's stream at the highest priority on top of that changed nothing at
// (32, 10000, 80) -- 1.6145 / 1.6129 / 1.6154 ms with both, this one, neither -- and took a tenth off the first scan's
// rate at (64, 30000, 100): not done.)  false = not available: the launches of round 3.
static bool early_setup(ivfhnsw_gpu *h)
{
    if (h->early_stream)
        return true;
    if (h->early_failed)
        return false;
    int least = 0, greatest = 0;
    hipStream_t s = nullptr;
    bool ok = hipDeviceGetStreamPriorityRange(&least, &greatest) == hipSuccess &&
              hipStreamCreateWithPriority(&s, hipStreamNonBlocking, least) == hipSuccess;
    for (int i = 0; i < 2 && ok; i++)
        ok = hipEventCreateWithFlags(&h->early_ready[i], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&h->early_done[i], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        (void)hipGetLastError();
        if (s)
            (void)hipStreamDestroy(s);
        h->early_failed = true; // (events that were created go with the handle)
        return false;
    }
    h->early_stream = s;
    return true;
}

static int search_dev_split(ivfhnsw_gpu *h, const SearchArgs &a, SearchCall &call)
{
    const size_t nq = a.nq;
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->split_view) {
        if ((rc = ivfhnsw_gpu_create_view(h, &h->split_view)))
            return rc;
        HIP_TRY(hipEventCreateWithFlags(&h->split_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&h->split_join, hipEventDisableTiming));
    }
    ivfhnsw_gpu *v = h->split_view;
    // the view follows the handle's tables (uploads since its creation included)
    follow_parent(v, h);
    v->profiling = h->profiling;
    v->status_shared = &status_words(h)->bits;
    // the second part: ~22 % of the batch, in whole "rounds" of the scan's resident workgroups (8 per CU x 256 CUs): its
    // scan runs alone at the end of the step, and 2200 workgroups on 2048 slots would take two rounds for one
    // (with early tables too: second parts of 1024 / 1536 / 2048 / 2560 queries, the short ones scanned by two workgroups
    // per query, gave 1.675 / 1.640 / 1.613 / 1.631 ms per step at (32, 10000, 80))
    const size_t round_wgs = 2048;
    auto second_part = [&](bool early_tables) {
        const int pm = h->split_pm == kSplitAuto ? auto_split_permille(h, a.p, early_tables) : h->split_pm;
        const size_t n = ((nq * (size_t)(1000 - pm) / 1000 + round_wgs / 2) / round_wgs) * round_wgs;
        return std::max(round_wgs, std::min(n, nq / 2));
    };
    // early tables where the second walk leaves resident slots to build them in (early_tables_wanted)
    const bool early = early_tables_wanted(h, a) && second_part(true) < (size_t)coarse_slots_for((int)a.p->efSearch) &&
                       early_setup(h);
    const size_t n2 = second_part(early), n1 = nq - n2;
    HIP_TRY(hipEventRecord(h->split_fork, h->stream));
    HIP_TRY(hipStreamWaitEvent(v->stream, h->split_fork, 0));
    EarlyTables part[2];
    if (early) {
        HIP_TRY(hipStreamWaitEvent(h->early_stream, h->split_fork, 0));
        for (int i = 0; i < 2; i++)
            part[i] = {h->early_stream, h->early_ready[i], h->early_done[i]};
    }
    call.early = early ? &part[0] : nullptr;
    rc = search_dev_chunk(h, a.slice(0, n1, (size_t)h->t.d), call);
    call.early = early ? &part[1] : nullptr;
    int rc2 = rc ? rc : search_dev_chunk(v, a.slice(n1, n2, (size_t)h->t.d), call);
    call.early = nullptr;
    // (whatever the second part flags it raises in the handle's own status word: v->status_shared)
    // the join itself, always (the fork was recorded)
    (void)hipSetDevice(h->device);
    if (early && rc2) {
        // a part failed on its way: its table launch may be out with no scan waiting for it.  (Otherwise each chain waits
        // for its tables in front of its scan, and the second part's are the last thing the helper stream was given.)
        HIP_TRY(hipEventRecord(h->early_done[1], h->early_stream));
        HIP_TRY(hipStreamWaitEvent(h->stream, h->early_done[1], 0));
    }
    HIP_TRY(hipEventRecord(h->split_join, v->stream));
    HIP_TRY(hipStreamWaitEvent(h->stream, h->split_join, 0));
    h->last_split = rc2 == 0;
    h->last_parts[0] = n1;
    h->last_parts[1] = n2;
    return rc2;
}

static int search_dev_part(ivfhnsw_gpu *h, const SearchArgs &a, SearchCall &call)
{
    if (h) {
        h->last_split = false;
        h->last_parts[0] = a.nq;
        h->last_parts[1] = 0;
    }
    const bool split = h && a.p && !h->is_view && h->split_pm > 0 && a.nq >= kSplitMinNq && !a.d_coarse_ids &&
                       !a.d_out_keys && !(a.p->heap_order && a.k > 1) && h->has_ivf && h->has_graph && a.p->nprobe > 0 &&
                       a.k > 0 && a.k <= 1024 && a.d_queries && a.d_distances && a.d_labels;
    return split ? search_dev_split(h, a, call) : search_dev_chunk(h, a, call);
}

static int search_dev_impl(ivfhnsw_gpu *h, const SearchArgs &a, SearchCall &call)
{
    const size_t kMaxBatch = (a.p && a.p->heap_order && a.k > 1) ? kMaxBatchAll / 8 : kMaxBatchAll;
    if (a.nq <= kMaxBatch || !h || !a.p)
        return search_dev_part(h, a, call);
    if (a.d_out_keys)
        return fail(IVFHNSW_ERR_INVALID, "sharded search (out_keys) is limited to %zu queries per call", kMaxBatch);
    for (size_t q0 = 0; q0 < a.nq; q0 += kMaxBatch) {
        int rc = search_dev_part(h, a.slice(q0, std::min(kMaxBatch, a.nq - q0), (size_t)h->t.d), call);
        if (rc)
            return rc;
    }
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_search_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                           const float *d_coarse_dists, const ivfhnsw_search_params *p, float *d_distances,
                           int64_t *d_labels, int64_t *d_out_keys)
{
    SearchCall call;
    return search_dev_impl(h, {nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, d_distances, d_labels, d_out_keys}, call);
}

// The same call with a filter slot, a tag (3.21), a value interval (3.24) or both (3.26) per query.  None is read
// back: a byte that names no installed slot, like a tag no row carries or an interval no row's value lies in, passes
// nothing.  An empty pick: the plain call.
static int search_pick_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                           const float *d_coarse_dists, const ivfhnsw_search_params *p, const QueryPick &pick,
                           float *d_distances, int64_t *d_labels, int64_t *d_out_keys)
{
    if (!pick)
        return ivfhnsw_gpu_search_dev(h, nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, d_distances, d_labels, d_out_keys);
    int rc = bind(h);
    if (rc || (rc = search_args_guard(h, p, k)) ||
        (rc = slots_call_guard(h, pick.who("search_slots_dev", "search_tags_dev", "search_values_dev", "search_tags_values_dev"), pick.kind())))
        return rc;
    if ((uintptr_t)pick.tags & 1)
        return fail(IVFHNSW_ERR_INVALID, "%s: query tags must be 2-byte aligned", pick.who("", "search_tags_dev", "", "search_tags_values_dev"));
    if ((uintptr_t)pick.ranges & 7)
        return fail(IVFHNSW_ERR_INVALID, "%s: query ranges must be 8-byte aligned", pick.who("", "", "search_values_dev", "search_tags_values_dev"));
    SearchCall call;
    return search_dev_impl(h, {nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, d_distances, d_labels, d_out_keys, pick}, call);
}

int ivfhnsw_gpu_search_slots_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                 const float *d_coarse_dists, const ivfhnsw_search_params *p, const uint8_t *d_query_slots,
                                 float *d_distances, int64_t *d_labels, int64_t *d_out_keys)
{
    return search_pick_dev(h, nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{d_query_slots, nullptr}, d_distances,
                           d_labels, d_out_keys);
}

int ivfhnsw_gpu_search_tags_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                const float *d_coarse_dists, const ivfhnsw_search_params *p, const uint16_t *d_query_tags,
                                float *d_distances, int64_t *d_labels, int64_t *d_out_keys)
{
    return search_pick_dev(h, nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{nullptr, d_query_tags}, d_distances,
                           d_labels, d_out_keys);
}

int ivfhnsw_gpu_search_values_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                  const float *d_coarse_dists, const ivfhnsw_search_params *p, const uint32_t *d_query_ranges,
                                  float *d_distances, int64_t *d_labels, int64_t *d_out_keys)
{
    return search_pick_dev(h, nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{nullptr, nullptr, d_query_ranges},
                           d_distances, d_labels, d_out_keys);
}

int ivfhnsw_gpu_search_tags_values_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                       const float *d_coarse_dists, const ivfhnsw_search_params *p, const uint16_t *d_query_tags,
                                       const uint32_t *d_query_ranges, float *d_distances, int64_t *d_labels, int64_t *d_out_keys)
{
    return search_pick_dev(h, nq, k, d_queries, d_coarse_ids, d_coarse_dists, p, QueryPick{nullptr, d_query_tags, d_query_ranges},
                           d_distances, d_labels, d_out_keys);
}

static void remember_plan(ivfhnsw_gpu *h, size_t nq, int max_seg, bool has_stream, const char *kernel_name)
{
    h->last_scan_kernel = kernel_name;
    h->last_nq = (int)nq;
    h->last_max_seg = max_seg;
    h->last_stream = has_stream;
}

int ivfhnsw_gpu_impl::chunk_checks(ivfhnsw_gpu *h, const Chunk &c, bool results)
{
    int rc = bind(h);
    if (rc || (rc = search_args_guard(h, c.p, c.k)))
        return rc;
    if ((c.d_coarse_ids == nullptr) != (c.d_coarse_dists == nullptr))
        return fail(IVFHNSW_ERR_INVALID, "coarse_ids and coarse_dists must both be given or both be NULL");
    if (c.nq > 0 && (!c.d_queries || (results && (!c.d_distances || !c.d_labels))))
        return fail(IVFHNSW_ERR_INVALID, "null query/result buffer");
    // k > 1024 only in heap order on the labels path: heap_scan_kernel, no stream
    if (c.k > 1024 && (!c.p->heap_order || c.d_out_keys))
        return fail(IVFHNSW_ERR_INVALID, "k %zu > 1024 unsupported (only heap_order = 1 without out_keys)", c.k);
    if (c.nq > 0x7fffffffull / (c.k > c.p->nprobe ? c.k : c.p->nprobe))
        return fail(IVFHNSW_ERR_INVALID, "nq too large");
    if (h->has_group && !h->has_graph)
        return fail(IVFHNSW_ERR_STATE, "Grouping search needs upload_quantizer (sub-centroid distances)");
    if (h->has_graph && (h->gr.d != h->t.d || h->gr.n != h->t.nc))
        return fail(IVFHNSW_ERR_STATE, "quantizer (%u x %d) does not match the index (%u x %d)", h->gr.n, h->gr.d,
                    h->t.nc, h->t.d);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_impl::chunk_workspace(ivfhnsw_gpu *h, Chunk &c)
{
    c.nprobe = (int)c.p->nprobe;
    c.max_seg = h->has_group ? c.nprobe * h->g.nsubc : c.nprobe;
    c.heap_big = c.k > 1024;
    c.plan_k = c.heap_big ? 1 : (int)c.k; // the plan kernels reset one key per query
    int rc;
    if ((rc = h->w_segs.ensure(c.nq * (size_t)c.max_seg * sizeof(Seg))) ||
        (rc = h->w_lpos.ensure(c.nq * (size_t)c.max_seg * sizeof(uint32_t))) ||
        (rc = h->w_hdr.ensure(c.nq * sizeof(PlanHdr))) ||
        (rc = h->w_keys.ensure(c.nq * (size_t)c.plan_k * sizeof(uint64_t))) ||
        (rc = h->w_totals.ensure(2 * sizeof(unsigned long long))))
        return rc;
    if (c.pick.both()) // both row arrays, either null without its table, and this chunk's tags and pairs
        c.fmask = TagValueMask{h->row_tags, h->row_values, c.pick.tags, c.pick.ranges};
    else if (c.pick.ranges) // the row values the handle (a view: its parent) holds, null without a table, and this chunk's pairs
        c.fmask = ValueMask{h->row_values, c.pick.ranges};
    else if (c.pick.tags) // the row tags the handle (a view: its parent) holds, null without a tag table, and this chunk's tags
        c.fmask = TagMask{h->row_tags, c.pick.tags};
    else if (c.pick.slots) // the planes the handle (a view: its parent) holds -- with none, any readable word: a query
                           // without a plane reads word 0 and ignores it -- and the bytes of this chunk's queries
        c.fmask = SlotMask{h->fs.nplanes ? h->fs.planes : h->w_totals.as<uint32_t>(), h->fs.stride, h->fs.nplanes, c.pick.slots};
    else
        c.fmask = h->filter.mode >= 0 ? h->fmask : nullptr;
    return IVFHNSW_OK;
}

// 1. rotate (IndexIVF_HNSW.cpp:240), 2. coarse (IndexIVF_HNSW.cpp:248-259)
int ivfhnsw_gpu_impl::chunk_coarse(ivfhnsw_gpu *h, Chunk &c, const SearchCall &call)
{
    const size_t nq = c.nq;
    int rc;
    c.xq = c.d_queries;
    if (h->t.opq_At) {
        if ((rc = h->w_xq.ensure(nq * (size_t)h->t.d * sizeof(float))))
            return rc;
        {
            StageScope sc(h, IVFHNSW_STAGE_OPQ);
            HIP_TRY(launch_opq(h->stream, h->t.opq_At, c.d_queries, h->w_xq.as<float>(), (int)nq, h->t.d));
        }
        c.xq = h->w_xq.as<float>();
        if (call.early) { // a split call's part: its tables are built from these, beside the walk that is launched next
            HIP_TRY(hipEventRecord(call.early->ready, h->stream));
            HIP_TRY(hipStreamWaitEvent(call.early->stream, call.early->ready, 0));
        }
    }
    // small IVFADC batches: everything behind the coarse stage in one launch (kernels_tail.hip); its per-query
    // meeting words are cleared by the latency walk when that runs, by a memset otherwise.  The one-launch tail and the
    // pipelined scan have no filtered form.
    static const size_t tail_max_nq = env_size("IVFHNSW_TAIL_MAX_NQ", 8);
    c.use_tail = !h->has_group && nq <= tail_max_nq && !c.d_out_keys && !c.fmask.any() &&
                 ivf_tail_supported(h->t, c.nprobe, (int)c.k);
    if (c.use_tail) {
        if ((rc = h->w_tail.ensure(nq * (sizeof(uint64_t) + sizeof(uint32_t)))))
            return rc;
        c.meet.keys = h->w_tail.as<uint64_t>();
        c.meet.done = reinterpret_cast<uint32_t *>(c.meet.keys + nq);
    }
    c.cid = c.d_coarse_ids;
    c.cd = c.d_coarse_dists;
    if (!c.cid) {
        if ((rc = h->w_cid.ensure(nq * (size_t)c.nprobe * sizeof(uint32_t))) ||
            (rc = h->w_cd.ensure(nq * (size_t)c.nprobe * sizeof(float))) ||
            (rc = coarse_dev_impl(h, nq, c.xq, c.p->nprobe, c.p->efSearch, h->w_cid.as<uint32_t>(), h->w_cd.as<float>(),
                                  call, c.meet)))
            return rc;
        c.cid = h->w_cid.as<uint32_t>();
        c.cd = h->w_cd.as<float>();
    }
    return IVFHNSW_OK;
}

static int chunk_tail(ivfhnsw_gpu *h, const Chunk &c, SearchCall &call)
{
    const size_t nq = c.nq;
    const int nsplit = (int)std::min<size_t>(32, (2048 + nq - 1) / nq);
    StageScope sc(h, IVFHNSW_STAGE_SCAN);
    if (!c.meet.cleared)
        HIP_TRY(hipMemsetAsync(c.meet.keys, 0, nq * (sizeof(uint64_t) + sizeof(uint32_t)), h->stream));
    HIP_TRY(launch_ivf_tail(h->stream, h->t, c.xq, c.cid, c.cd, (int)nq, c.nprobe, c.p->max_codes, nsplit, c.meet.keys,
                            c.meet.done, h->w_hdr.as<PlanHdr>(), c.d_distances, c.d_labels, status_word(h),
                            call.status_out));
    call.wrote_status = call.status_out != nullptr;
    remember_plan(h, nq, c.max_seg, false, "ivf_tail_kernel");
    return IVFHNSW_OK;
}

// 3. plan (IndexIVF_HNSW.cpp:267-292 / IndexIVF_HNSW_Grouping.cpp:222-353), 4. table (IndexIVF_HNSW.cpp:262)
int ivfhnsw_gpu_impl::chunk_plan_table(ivfhnsw_gpu *h, Chunk &c)
{
    const int nq = (int)c.nq, max_seg = c.max_seg;
    const ivfhnsw_search_params *p = c.p;
    int rc;
    c.heap = p->heap_order && c.k > 1;
    // small batches: split each query over several workgroups so the chip still fills
    c.nsplit = (c.k == 1 && c.nq < 1024) ? (int)std::min<size_t>(32, (2048 + c.nq - 1) / c.nq) : 1;
    // list shards: table and scan in one software-pipelined kernel, the table never leaves the chip (kernels_scan3.hip)
    c.pipe = c.k == 1 && !h->has_group && !c.heap && !c.fmask.any() && h->opt_scan_pipe != 0 &&
             scan_pipe_supported(h->t, max_seg, nq, c.nsplit, h->n_local > 0, h->opt_scan_pipe == 1);
    const bool plan_lut = !c.pipe && plan_lut_shape(h);
    if (!c.pipe && (rc = h->w_luts.ensure(c.nq * (size_t)h->t.M * 256 * sizeof(float))))
        return rc;
    const PlanView plan = plan_of(h, max_seg, c.nq);
    uint64_t *keys = h->w_keys.as<uint64_t>();
    if (plan_lut && c.early) {
        // A split call's part: the tables need only the (rotated) queries, so they are built on the helper stream, into
        // this part's own w_luts, while the walks run -- launched here, behind the walk in host order, so that the walk's
        // wavefronts are on the chip first and the table workgroups (lowest priority) take slots that walks have left.
        // This stream then runs the plan alone and meets the tables in front of the scan.  (The wait in front of the plan
        // instead: 1.6037 against 1.6072 ms per step, inside the run-to-run spread.)
        const EarlyTables &e = *c.early;
        {
            StageScope sc(h, IVFHNSW_STAGE_LUT, e.stream);
            HIP_TRY(launch_lut(e.stream, h->t, c.xq, h->w_luts.as<float>(), nq, nullptr));
        }
        HIP_TRY(hipEventRecord(e.done, e.stream));
        {
            StageScope sc(h, IVFHNSW_STAGE_PLAN);
            HIP_TRY(launch_plan_ivf(h->stream, h->t, c.cid, c.cd, c.nprobe, p->max_codes, plan, keys, c.plan_k));
        }
        HIP_TRY(hipStreamWaitEvent(h->stream, e.done, 0));
        return IVFHNSW_OK;
    }
    if (plan_lut) {
        StageScope sc(h, IVFHNSW_STAGE_LUT); // plan + tables: one kernel, accounted as the table stage
        HIP_TRY(launch_plan_lut(h->stream, h->t, c.xq, c.cid, c.cd, c.nprobe, p->max_codes, plan, keys, c.plan_k,
                                h->w_luts.as<float>()));
        return IVFHNSW_OK;
    }
    {
        StageScope sc(h, IVFHNSW_STAGE_PLAN);
        if (h->has_group) {
            // per query: pass-1 values and sub-centroid distances of every (row, sub-group) the plan touches
            if ((rc = h->w_qsd.ensure(c.nq * (size_t)max_seg * 2 * sizeof(float))))
                return rc;
            HIP_TRY(launch_plan_grouping(h->stream, h->t, h->g, h->gr, c.xq, c.cid, c.cd, c.nprobe, p->max_codes,
                                         p->do_pruning, plan, keys, c.plan_k, h->w_qsd.as<float>()));
        } else {
            HIP_TRY(launch_plan_ivf(h->stream, h->t, c.cid, c.cd, c.nprobe, p->max_codes, plan, keys, c.plan_k));
        }
    }
    if (!c.pipe) {
        StageScope sc(h, IVFHNSW_STAGE_LUT);
        HIP_TRY(launch_lut(h->stream, h->t, c.xq, h->w_luts.as<float>(), nq, plan.hdr));
    }
    return IVFHNSW_OK;
}

// 5. scan (IndexIVF_HNSW.cpp:282-289), 6. select
static int chunk_scan_select(ivfhnsw_gpu *h, const Chunk &c)
{
    const int k = (int)c.k;
    const bool heap = c.heap, replay_here = c.heap && !c.d_out_keys;
    float *luts = h->w_luts.as<float>();
    const PlanView plan = plan_of(h, c.max_seg, c.nq);
    int rc;
    // heap_scan_kernel's global-tier heaps (k beyond what fits in LDS beside the table) and its redo list
    float *heap_ws = nullptr;
    if (replay_here) {
        if ((rc = h->w_heap.ensure(heap_scan_ws_bytes(h->t.M, k, plan.nq))))
            return rc;
        heap_ws = h->w_heap.as<float>();
    }
    if (c.heap_big) {
        // scan and heap replay in one kernel, every query of the batch; no candidate stream exists
        {
            StageScope sc(h, IVFHNSW_STAGE_SCAN);
            HIP_TRY(launch_heap_scan(h->stream, h->t, luts, plan, k, nullptr, nullptr, heap_ws, c.d_distances, c.d_labels,
                                     c.fmask));
        }
        remember_plan(h, c.nq, c.max_seg, false, c.fmask.name("heap_scan_kernel", "heap_scan_kernel+filter", "heap_scan_kernel+slots", "heap_scan_kernel+tags", "heap_scan_kernel+values", "heap_scan_kernel+tags+values"));
        return IVFHNSW_OK;
    }
    if (heap) {
        // with out_keys (sharded search) the replay is the caller's: it merges the shards' candidate streams in scan
        // order first (ivfhnsw_gpu_last_stream_dev, ivfhnsw_gpu_replay_stream_dev)
        if ((rc = h->w_stream.ensure(c.nq * (size_t)kHeapStreamCap * sizeof(uint64_t))) ||
            (rc = h->w_slen.ensure(c.nq * sizeof(uint32_t))) ||
            (replay_here && (rc = h->w_hredo.ensure(c.nq * sizeof(uint32_t)))))
            return rc;
    }
    bool scan_selected = false;
    const char *kernel_name = "scan_pipe_kernel";
    {
        StageScope sc(h, IVFHNSW_STAGE_SCAN);
        if (c.pipe) {
            HIP_TRY(launch_scan_pipe(h->stream, h->t, c.xq, plan, h->w_keys.as<uint64_t>()));
        } else {
            // a plan segment is a list (IVFADC) or a sub-group (Grouping): the mean length decides the scan form
            const uint64_t nseg_all = (uint64_t)h->t.nc * (h->has_group ? (uint64_t)h->g.nsubc : 1);
            const int seg_hint =
                (int)std::min<uint64_t>(1u << 20, nseg_all ? (h->n_local * h->t.shard_world) / nseg_all : 0);
            ScanOut out;
            if (heap) {
                out.stream = h->w_stream.as<uint64_t>();
                out.stream_len = h->w_slen.as<uint32_t>();
                out.stream_cap = kHeapStreamCap;
            } else if (k == 1 && !c.d_out_keys) {
                // k = 1 without out_keys: the scan writes distance and label itself where it can (no select launch)
                out.sel_dist = c.d_distances;
                out.sel_labels = c.d_labels;
            }
            HIP_TRY(launch_scan(h->stream, h->t, luts, plan, k, c.nsplit, h->w_keys.as<uint64_t>(), seg_hint, c.fmask, out,
                                &scan_selected, &kernel_name));
        }
    }
    if (!scan_selected) {
        StageScope sc(h, IVFHNSW_STAGE_SELECT);
        if (replay_here) {
            // a query whose stream overflowed goes on the redo list instead of failing the batch; heap_scan_kernel redoes
            // it from the plan and the table.  Fixed grid, count read on the device: no host synchronisation, and an
            // empty list costs one launch that exits at once (its last workgroup re-zeroes the two heap_redo words)
            uint32_t *redo_hdr = &status_words(h)->heap_redo_len;
            HIP_TRY(launch_heap_replay(h->stream, h->t, plan, h->w_stream.as<uint64_t>(), h->w_slen.as<uint32_t>(),
                                       kHeapStreamCap, k, c.d_distances, c.d_labels, status_word(h), nullptr, redo_hdr,
                                       h->w_hredo.as<uint32_t>()));
            HIP_TRY(launch_heap_scan(h->stream, h->t, luts, plan, k, redo_hdr, h->w_hredo.as<uint32_t>(), heap_ws,
                                     c.d_distances, c.d_labels, c.fmask));
        } else
            HIP_TRY(launch_select(h->stream, h->t, plan, h->w_keys.as<uint64_t>(), k, c.d_distances, c.d_labels,
                                  c.d_out_keys));
    }
    remember_plan(h, c.nq, c.max_seg, heap, kernel_name);
    return IVFHNSW_OK;
}

static int search_dev_chunk(ivfhnsw_gpu *h, const SearchArgs &a, SearchCall &call)
{
    Chunk c{a};
    int rc = chunk_checks(h, c);
    if (rc)
        return rc;
    h->last_nq = 0;
    h->last_range = false;
    call.wrote_status = false;
    if (c.nq == 0)
        return IVFHNSW_OK;
    c.early = call.early;
    if ((rc = chunk_workspace(h, c)) || (rc = chunk_coarse(h, c, call)))
        return rc;
    if (c.use_tail)
        return chunk_tail(h, c, call);
    if ((rc = chunk_plan_table(h, c)))
        return rc;
    return chunk_scan_select(h, c);
}

int ivfhnsw_gpu_resolve_keys_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const int64_t *d_keys, float *d_distances,
                                 int64_t *d_labels)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_ivf || h->last_nq == 0 || (size_t)h->last_nq != nq || h->last_range)
        return fail(IVFHNSW_ERR_STATE, "resolve_keys needs the plan of a preceding search_dev with the same nq");
    StageScope sc(h, IVFHNSW_STAGE_SELECT);
    HIP_TRY(launch_resolve(h->stream, h->t, plan_of(h, h->last_max_seg, nq), d_keys, (int)k, d_distances, d_labels));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_last_stream_dev(ivfhnsw_gpu *h, size_t nq, size_t len_cap, uint64_t *d_keys, uint32_t *d_len,
                                uint32_t *stream_cap)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->last_nq || !h->last_stream || (size_t)h->last_nq != nq)
        return fail(IVFHNSW_ERR_STATE, "last_stream needs a preceding search_dev of the same nq with k > 1 and heap_order = 1");
    if (stream_cap)
        *stream_cap = kHeapStreamCap;
    if (d_len)
        HIP_TRY(hipMemcpyAsync(d_len, h->w_slen.p, nq * sizeof(uint32_t), hipMemcpyDeviceToDevice, h->stream));
    if (d_keys) {
        if (len_cap == 0 || len_cap > kHeapStreamCap)
            return fail(IVFHNSW_ERR_INVALID, "len_cap %zu outside 1..%u", len_cap, kHeapStreamCap);
        HIP_TRY(hipMemcpy2DAsync(d_keys, len_cap * sizeof(uint64_t), h->w_stream.p, (size_t)kHeapStreamCap * sizeof(uint64_t),
                                 len_cap * sizeof(uint64_t), nq, hipMemcpyDeviceToDevice, h->stream));
    }
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_replay_stream_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const uint64_t *d_stream, const uint32_t *d_len,
                                  uint32_t cap, int64_t *d_out_keys)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (!h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "replay_stream before upload_ivf");
    if (nq == 0)
        return IVFHNSW_OK;
    if (!d_stream || !d_len || !d_out_keys || k == 0 || k > 1024 || nq > 0x7fffffffull / k)
        return fail(IVFHNSW_ERR_INVALID, "bad replay_stream arguments (k %zu)", k);
    StageScope sc(h, IVFHNSW_STAGE_SELECT);
    // no plan: with out_keys the replay resolves no labels
    HIP_TRY(launch_heap_replay(h->stream, h->t, PlanView{nullptr, nullptr, nullptr, 0, (int)nq}, d_stream, d_len, cap, (int)k,
                               nullptr, nullptr, status_word(h), d_out_keys));
    return IVFHNSW_OK;
}

// ivfhnsw_gpu_search, and with a pick (a slot byte, a tag or an interval per query, host memory) ivfhnsw_gpu_search_slots /
// _tags / _values: the bytes ride in the pinned input block or a staging buffer beside the queries
static int search_host(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                       const float *coarse_dists, const ivfhnsw_search_params *p, const QueryPick &pick, float *distances,
                       int64_t *labels)
{
    int rc = bind(h);
    if (rc || (rc = search_args_guard(h, p, k)))
        return rc;
    const char *who = pick.who("search_slots", "search_tags", "search_values", "search_tags_values");
    if (pick && (rc = slots_call_guard(h, who, pick.kind())))
        return rc;
    if (nq == 0)
        return IVFHNSW_OK;
    if (!queries || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "null query/result buffer");
    if ((coarse_ids == nullptr) != (coarse_dists == nullptr))
        return fail(IVFHNSW_ERR_INVALID, "coarse_ids and coarse_dists must both be given or both be NULL");
    if (pick.slots && (rc = slots_bytes_guard(nq, pick.slots, who)))
        return rc;
    const size_t in_q = nq * h->t.d * sizeof(float), in_c = coarse_ids ? nq * p->nprobe * sizeof(uint32_t) : 0;
    const size_t in_s = pick.bytes(nq);
    // Small batches -- the reference's drivers pass ONE query per call (tests/test_ivfhnsw_sift1b.cpp:193-208) -- go
    // through pinned host memory the kernels read and write directly: no staging copies, one synchronisation.  Layout
    // of the two blocks: in = queries | coarse ids | coarse dists | the pick's arrays, at the next multiple of 8 (a _values
    // call's pairs are 8-byte aligned wherever they come from; a _tags_values call's tags follow its pairs); out = distances | labels | status word.
    static const size_t pinned_max_nq = env_size("IVFHNSW_PINNED_MAX_NQ", 256);
    if (nq <= pinned_max_nq) {
        const size_t out_d = (nq * k * sizeof(float) + 7) & ~(size_t)7, out_l = nq * k * sizeof(int64_t);
        const size_t at_s = (in_q + 2 * in_c + 7) & ~(size_t)7;
        if ((rc = h->p_in.ensure(at_s + in_s)) || (rc = h->p_out.ensure(out_d + out_l + 8)))
            return rc;
        char *pin = h->p_in.as<char>(), *pout = h->p_out.as<char>();
        memcpy(pin, queries, in_q);
        if (coarse_ids) {
            memcpy(pin + in_q, coarse_ids, in_c);
            memcpy(pin + in_q + in_c, coarse_dists, in_c);
        }
        pick.each_array(nq, [&](const void *src, size_t at, size_t bytes) {
            memcpy(pin + at_s + at, src, bytes);
            return 0;
        });
        uint32_t *pst = reinterpret_cast<uint32_t *>(pout + out_d + out_l);
        uint32_t *bits = &status_words(h)->bits;
        // The latency walk keeps at most 64 exact ties at the efSearch boundary.  This call synchronises anyway, so instead
        // of a redo launch behind every one-query call the walk only raises a status bit, and the call repeats itself once
        // on the throughput walk, whose redo form has no such limit (hnswalg.cpp:67-68,93 has none either).
        for (int attempt = 0; attempt < 2; attempt++) {
            SearchCall call{pst, attempt == 0, attempt == 1};
            rc = search_dev_impl(h,
                                 {nq, k, reinterpret_cast<const float *>(pin),
                                  coarse_ids ? reinterpret_cast<const uint32_t *>(pin + in_q) : nullptr,
                                  coarse_ids ? reinterpret_cast<const float *>(pin + in_q + in_c) : nullptr, p,
                                  reinterpret_cast<float *>(pout), reinterpret_cast<int64_t *>(pout + out_d), nullptr,
                                  pick.at(pin + at_s, nq)},
                                 call);
            if (rc)
                return rc;
            if (!call.wrote_status)
                HIP_TRY(hipMemcpyAsync(pst, bits, sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
            HIP_TRY(hipStreamSynchronize(h->stream));
            if (attempt == 0 && (*pst & kStatusHnswTieOverflow)) {
                *pst &= ~kStatusHnswTieOverflow;
                HIP_TRY(hipMemcpy(bits, pst, sizeof(uint32_t), hipMemcpyHostToDevice)); // bit consumed
                continue;
            }
            break;
        }
        memcpy(distances, pout, nq * k * sizeof(float));
        memcpy(labels, pout + out_d, out_l);
        return *pst ? check_status(h) : IVFHNSW_OK;
    }
    if ((rc = h->s_dist.ensure(nq * k * sizeof(float))) || (rc = h->s_lab.ensure(nq * k * sizeof(int64_t))) ||
        (rc = stage_in(h, h->s_q, queries, in_q)) ||
        (coarse_ids && ((rc = stage_in(h, h->s_cid, coarse_ids, in_c)) || (rc = stage_in(h, h->s_cd, coarse_dists, in_c)))) ||
        (pick && (rc = pick_stage_in(h, pick, nq))) ||
        (rc = search_pick_dev(h, nq, k, h->s_q.as<float>(), coarse_ids ? h->s_cid.as<uint32_t>() : nullptr,
                              coarse_ids ? h->s_cd.as<float>() : nullptr, p, pick.at(h->fs_qslots.p, nq), h->s_dist.as<float>(),
                              h->s_lab.as<int64_t>(), nullptr)) ||
        (rc = stage_out(h, distances, h->s_dist, nq * k * sizeof(float))) ||
        (rc = stage_out(h, labels, h->s_lab, nq * k * sizeof(int64_t))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return check_status(h);
}

int ivfhnsw_gpu_search(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                       const float *coarse_dists, const ivfhnsw_search_params *p, float *distances, int64_t *labels)
{
    return search_host(h, nq, k, queries, coarse_ids, coarse_dists, p, QueryPick{}, distances, labels);
}

int ivfhnsw_gpu_search_slots(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                             const float *coarse_dists, const ivfhnsw_search_params *p, const uint8_t *query_slots,
                             float *distances, int64_t *labels)
{
    return search_host(h, nq, k, queries, coarse_ids, coarse_dists, p, QueryPick{query_slots, nullptr}, distances, labels);
}

int ivfhnsw_gpu_search_tags(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                            const float *coarse_dists, const ivfhnsw_search_params *p, const uint16_t *query_tags,
                            float *distances, int64_t *labels)
{
    return search_host(h, nq, k, queries, coarse_ids, coarse_dists, p, QueryPick{nullptr, query_tags}, distances, labels);
}

int ivfhnsw_gpu_search_values(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                              const float *coarse_dists, const ivfhnsw_search_params *p, const uint32_t *query_ranges,
                              float *distances, int64_t *labels)
{
    return search_host(h, nq, k, queries, coarse_ids, coarse_dists, p, QueryPick{nullptr, nullptr, query_ranges}, distances, labels);
}

int ivfhnsw_gpu_search_tags_values(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                                   const float *coarse_dists, const ivfhnsw_search_params *p, const uint16_t *query_tags,
                                   const uint32_t *query_ranges, float *distances, int64_t *labels)
{
    return search_host(h, nq, k, queries, coarse_ids, coarse_dists, p, QueryPick{nullptr, query_tags, query_ranges}, distances, labels);
}

int ivfhnsw_gpu_search_keys(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                            const float *coarse_dists, const ivfhnsw_search_params *p, int64_t *keys)
{
    int rc = bind(h);
    if (rc || (rc = search_args_guard(h, p, k)))
        return rc;
    if (nq == 0)
        return IVFHNSW_OK;
    if (!queries || !keys || !coarse_ids || !coarse_dists)
        return fail(IVFHNSW_ERR_INVALID, "null buffer (a shard is searched with the coarse stage supplied)");
    const size_t d = h->t.d, np = p->nprobe;
    if ((rc = h->s_dist.ensure(nq * k * sizeof(float))) || (rc = h->s_lab.ensure(nq * k * sizeof(int64_t))) ||
        (rc = h->s_keys.ensure(nq * k * sizeof(int64_t))) || (rc = stage_in(h, h->s_q, queries, nq * d * sizeof(float))) ||
        (rc = stage_in(h, h->s_cid, coarse_ids, nq * np * sizeof(uint32_t))) ||
        (rc = stage_in(h, h->s_cd, coarse_dists, nq * np * sizeof(float))) ||
        (rc = ivfhnsw_gpu_search_dev(h, nq, k, h->s_q.as<float>(), h->s_cid.as<uint32_t>(), h->s_cd.as<float>(), p,
                                     h->s_dist.as<float>(), h->s_lab.as<int64_t>(), h->s_keys.as<int64_t>())) ||
        (rc = stage_out(h, keys, h->s_keys, nq * k * sizeof(int64_t))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return check_status(h);
}

int ivfhnsw_gpu_resolve_keys(ivfhnsw_gpu *h, size_t nq, size_t k, const int64_t *keys, float *distances, int64_t *labels)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (nq == 0)
        return IVFHNSW_OK;
    if (!keys || !distances || !labels)
        return fail(IVFHNSW_ERR_INVALID, "null buffer");
    if ((rc = h->s_dist.ensure(nq * k * sizeof(float))) || (rc = h->s_lab.ensure(nq * k * sizeof(int64_t))) ||
        (rc = stage_in(h, h->s_keys, keys, nq * k * sizeof(int64_t))) ||
        (rc = ivfhnsw_gpu_resolve_keys_dev(h, nq, k, h->s_keys.as<int64_t>(), h->s_dist.as<float>(), h->s_lab.as<int64_t>())) ||
        (rc = stage_out(h, distances, h->s_dist, nq * k * sizeof(float))) ||
        (rc = stage_out(h, labels, h->s_lab, nq * k * sizeof(int64_t))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_last_stream(ivfhnsw_gpu *h, size_t nq, size_t len_cap, uint64_t *keys, uint32_t *lens, uint32_t *stream_cap)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (lens && ((rc = h->s_len.ensure(nq * sizeof(uint32_t))) ||
                 (rc = ivfhnsw_gpu_last_stream_dev(h, nq, 0, nullptr, h->s_len.as<uint32_t>(), stream_cap)) ||
                 (rc = stage_out(h, lens, h->s_len, nq * sizeof(uint32_t)))))
        return rc;
    if (keys && ((rc = h->s_keys.ensure(nq * len_cap * sizeof(uint64_t))) ||
                 (rc = ivfhnsw_gpu_last_stream_dev(h, nq, len_cap, h->s_keys.as<uint64_t>(), nullptr, stream_cap)) ||
                 (rc = stage_out(h, keys, h->s_keys, nq * len_cap * sizeof(uint64_t)))))
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return IVFHNSW_OK;
}
