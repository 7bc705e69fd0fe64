// The handle of the C ABI (include/ivfhnsw_hip.h): its life, views, stream, options, stage timers and accounting, and the
// helpers every other capi_*.cpp shares (capi_internal.h).
#include "capi_internal.h"

#include <cstdarg>

static thread_local std::string g_last_error;

namespace ivfhnsw_gpu_impl {

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
    return code;
}

int bind(ivfhnsw_gpu *h)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    HIP_TRY(hipSetDevice(h->device));
    return IVFHNSW_OK;
}

int upload(DevBuf &b, const void *src, size_t bytes)
{
    int rc = b.ensure(bytes);
    if (rc)
        return rc;
    if (bytes)
        HIP_TRY(hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
    return IVFHNSW_OK;
}

hipEvent_t take_event(ivfhnsw_gpu *h)
{
    if (!h->pool.empty()) {
        hipEvent_t e = h->pool.back();
        h->pool.pop_back();
        return e;
    }
    hipEvent_t e = nullptr;
    (void)hipEventCreate(&e);
    return e;
}

int drain_events(ivfhnsw_gpu *h)
{
    for (auto &ev : h->pending) {
        HIP_TRY(hipEventSynchronize(ev.b));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, ev.a, ev.b));
        h->stage_ms[ev.stage] += ms;
        h->stage_n[ev.stage] += 1;
        h->pool.push_back(ev.a);
        h->pool.push_back(ev.b);
    }
    h->pending.clear();
    return IVFHNSW_OK;
}

int check_status(ivfhnsw_gpu *h)
{
    uint32_t st = 0;
    HIP_TRY(hipMemcpy(&st, &status_words(h)->bits, sizeof(st), hipMemcpyDeviceToHost));
    if (!st)
        return IVFHNSW_OK;
    HIP_TRY(hipMemset(&status_words(h)->bits, 0, sizeof(st)));
    if (st & kStatusHnswTieOverflow)
        return fail(IVFHNSW_ERR_STATE, "HNSW walk: more than 64 candidates tie exactly with the efSearch-th "
                                       "distance; results of this batch are invalid");
    if (st & kStatusTopkStreamOverflow)
        return fail(IVFHNSW_ERR_STATE, "heap-order top-k: candidate stream of a query exceeded %u entries; use "
                                       "heap_order = 0 for this k / max_codes", kHeapStreamCap);
    return fail(IVFHNSW_ERR_STATE, "device status 0x%x", st);
}

void follow_parent(ivfhnsw_gpu *view, const ivfhnsw_gpu *parent)
{
    view->t = parent->t;
    view->opq_A = parent->opq_A;
    view->has_ivf = parent->has_ivf;
    view->n_local = parent->n_local;
    view->g = parent->g;
    view->has_group = parent->has_group;
    view->gr = parent->gr;
    view->has_graph = parent->has_graph;
    view->filter.mode = parent->filter.mode; // the view filters as its parent does at this moment
    view->fmask = parent->fmask;
    view->filter.pass = parent->filter.pass; // (mode and count only: the bitmap stays the parent's)
    view->fs = parent->fs; // ... and reads the filter slots its parent holds
    view->row_tags = parent->row_tags; // ... and its row tags (3.21)
    view->tg_labels = parent->tg_labels;
    view->row_values = parent->row_values; // ... and its row values (3.24)
    view->vl_labels = parent->vl_labels;
}

int table_change_guard(ivfhnsw_gpu *h, TableChange what, const char *who, bool need_ivf)
{
    if (h && h->is_view) {
        static const char *const kinds[] = {"uploads", "appends", "removals"};
        return fail(IVFHNSW_ERR_STATE, "%s%s%s go to the handle that holds the tables, not to a view of it",
                    what == kUploads ? "" : who, what == kUploads ? "" : ": ", kinds[what]);
    }
    int rc = bind(h);
    if (rc)
        return rc;
    if (need_ivf && !h->has_ivf)
        return fail(IVFHNSW_ERR_STATE, "%s before upload_ivf", who);
    return IVFHNSW_OK;
}

void point_at_lists(ivfhnsw_gpu *h, uint64_t n_local)
{
    h->t.goff = h->goff.as<uint64_t>();
    h->t.loff = h->loff.as<uint32_t>();
    h->t.codes = h->codes.as<uint8_t>();
    h->t.norm_codes = h->ncodes.as<uint8_t>();
    h->t.ids = h->ids.as<uint32_t>();
    h->n_local = n_local;
}

} // namespace ivfhnsw_gpu_impl

const char *ivfhnsw_gpu_last_error(void) { return g_last_error.c_str(); }

int ivfhnsw_gpu_abi_version(void) { return 9; }

int ivfhnsw_gpu_device_count(int *count)
{
    if (!count)
        return fail(IVFHNSW_ERR_INVALID, "null argument");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess)
        return fail(IVFHNSW_ERR_HIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
    *count = n;
    return IVFHNSW_OK;
}

static int split_permille_env()
{
    static const int v = [] {
        // on by default since round 3; IVFHNSW_SPLIT=0 = one part, 1..999 = that share in the first part, unset = by estimate
        const char *e = getenv("IVFHNSW_SPLIT");
        const int x = (e && *e) ? atoi(e) : kSplitAuto;
        return (x > 0 && x <= kSplitAuto) ? x : 0;
    }();
    return v;
}

int ivfhnsw_gpu_create(int device, ivfhnsw_gpu **out)
{
    if (!out)
        return fail(IVFHNSW_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0)
        return fail(IVFHNSW_ERR_HIP, "no HIP device available (%s); there is no CPU fallback",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device < 0 || device >= ndev)
        return fail(IVFHNSW_ERR_INVALID, "device %d out of range (have %d)", device, ndev);
    HIP_TRY(hipSetDevice(device));
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(IVFHNSW_ERR_HIP, "device %d is %s; this library holds gfx950 code only", device, prop.gcnArchName);
    ivfhnsw_gpu *h = new ivfhnsw_gpu();
    h->device = device;
    hipError_t se = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
    if (se != hipSuccess) {
        delete h;
        return fail(IVFHNSW_ERR_HIP, "hipStreamCreate: %s", hipGetErrorString(se));
    }
    h->own_stream = true;
    h->split_pm = split_permille_env();
    if (h->w_status.ensure(sizeof(StatusWords)) || hipMemset(h->w_status.p, 0, sizeof(StatusWords)) != hipSuccess) {
        ivfhnsw_gpu_destroy(h);
        return fail(IVFHNSW_ERR_HIP, "cannot allocate the device status word");
    }
    *out = h;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_destroy(ivfhnsw_gpu *h)
{
    if (!h)
        return IVFHNSW_OK;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    if (h->split_view) {
        ivfhnsw_gpu_destroy(h->split_view);
        h->split_view = nullptr;
        (void)hipSetDevice(h->device);
    }
    if (h->split_fork)
        (void)hipEventDestroy(h->split_fork);
    if (h->split_join)
        (void)hipEventDestroy(h->split_join);
    if (h->early_stream) { // (joined into h->stream by every call that used it)
        (void)hipStreamSynchronize(h->early_stream);
        (void)hipStreamDestroy(h->early_stream);
    }
    for (hipEvent_t e : {h->early_ready[0], h->early_ready[1], h->early_done[0], h->early_done[1]})
        if (e)
            (void)hipEventDestroy(e);
    for (auto &ev : h->pending) {
        (void)hipEventDestroy(ev.a);
        (void)hipEventDestroy(ev.b);
    }
    for (auto e : h->pool)
        (void)hipEventDestroy(e);
    h->for_each_devbuf([](DevBuf &b) { b.release(); });
    h->p_in.release();
    h->p_out.release();
    if (h->own_stream)
        (void)hipStreamDestroy(h->stream);
    delete h;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_create_view(ivfhnsw_gpu *parent, ivfhnsw_gpu **out)
{
    if (!out)
        return fail(IVFHNSW_ERR_INVALID, "null out pointer");
    *out = nullptr;
    int rc = bind(parent);
    if (rc)
        return rc;
    if (parent->is_view)
        return fail(IVFHNSW_ERR_INVALID, "a view of a view: create it from the handle that holds the tables");
    // the parent's uploads (and the neighbour-row build) run on its stream: finished before anyone reads them
    HIP_TRY(hipStreamSynchronize(parent->stream));
    ivfhnsw_gpu *h = nullptr;
    if ((rc = ivfhnsw_gpu_create(parent->device, &h)))
        return rc;
    h->is_view = true;
    h->split_pm = 0;
    follow_parent(h, parent);
    h->parent = parent;
    *out = h;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_set_stream(ivfhnsw_gpu *h, void *hip_stream)
{
    int rc = bind(h);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    if (h->own_stream)
        (void)hipStreamDestroy(h->stream);
    h->stream = reinterpret_cast<hipStream_t>(hip_stream);
    h->own_stream = false;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_sync(ivfhnsw_gpu *h)
{
    int rc = bind(h);
    if (rc)
        return rc;
    HIP_TRY(hipStreamSynchronize(h->stream));
    return check_status(h);
}

int ivfhnsw_gpu_set_batch_split(ivfhnsw_gpu *h, int permille)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    if (permille < 0 || permille > kSplitAuto)
        return fail(IVFHNSW_ERR_INVALID, "batch split %d outside 0..999 permille (1000 = by estimate)", permille);
    if (h->is_view && permille)
        return fail(IVFHNSW_ERR_INVALID, "a view cannot split its batches (it is what the second part runs on)");
    h->split_pm = permille;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_set_option(ivfhnsw_gpu *h, const char *key, long value)
{
    if (!h || !key)
        return fail(IVFHNSW_ERR_INVALID, "set_option: null argument");
    if (!strcmp(key, "scan_pipe")) {
        if (value < -1 || value > 1)
            return fail(IVFHNSW_ERR_INVALID, "set_option scan_pipe: %ld outside -1..1", value);
        h->opt_scan_pipe = (int)value;
        return IVFHNSW_OK;
    }
    if (!strcmp(key, "exact_splits")) {
        if (value != -1 && (value < 1 || value > 64))
            return fail(IVFHNSW_ERR_INVALID, "set_option exact_splits: %ld is neither -1 nor in 1..64", value);
        h->opt_exact_splits = (int)value;
        return IVFHNSW_OK;
    }
    if (!strcmp(key, "exact_range_map")) {
        if (value < -1 || value > 1)
            return fail(IVFHNSW_ERR_INVALID, "set_option exact_range_map: %ld outside -1..1", value);
        h->opt_exact_range_map = (int)value;
        return IVFHNSW_OK;
    }
    if (!strcmp(key, "exact_filter_form")) {
        if (value < -1 || value > 1)
            return fail(IVFHNSW_ERR_INVALID, "set_option exact_filter_form: %ld outside -1..1", value);
        h->opt_exact_filter_form = (int)value;
        return base_slots_table_write(h, false); // the form of a base filter slot is the holder's choice
    }
    return fail(IVFHNSW_ERR_INVALID, "set_option: unknown key '%s'", key);
}

int ivfhnsw_gpu_set_profiling(ivfhnsw_gpu *h, int enabled)
{
    int rc = bind(h);
    if (rc)
        return rc;
    h->profiling = enabled == 2 ? 2 : (enabled != 0 ? 1 : 0);
    if (h->split_view)
        h->split_view->profiling = h->profiling;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_get_stage_ms(ivfhnsw_gpu *h, int stage, double *ms_total, uint64_t *launches)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if (stage < 0 || stage >= IVFHNSW_STAGE_COUNT)
        return fail(IVFHNSW_ERR_INVALID, "bad stage %d", stage);
    if ((rc = drain_events(h)))
        return rc;
    double ms = h->stage_ms[stage];
    uint64_t n = h->stage_n[stage];
    if (h->split_view) { // the second part of split batches: its launches and their time join the handle's
        if ((rc = drain_events(h->split_view)))
            return rc;
        ms += h->split_view->stage_ms[stage];
        n += h->split_view->stage_n[stage];
    }
    if (ms_total)
        *ms_total = ms;
    if (launches)
        *launches = n;
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_reset_stage_ms(ivfhnsw_gpu *h)
{
    int rc = bind(h);
    if (rc)
        return rc;
    if ((rc = drain_events(h)))
        return rc;
    for (int i = 0; i < IVFHNSW_STAGE_COUNT; i++) {
        h->stage_ms[i] = 0;
        h->stage_n[i] = 0;
    }
    if (h->split_view)
        return ivfhnsw_gpu_reset_stage_ms(h->split_view);
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_last_scan_counts(ivfhnsw_gpu *h, uint64_t *ncodes, uint64_t *nsegments)
{
    int rc = bind(h);
    if (rc)
        return rc;
    unsigned long long out[2] = {0, 0};
    if (h->last_nq) {
        HIP_TRY(launch_plan_totals(h->stream, h->w_hdr.as<PlanHdr>(), h->last_nq,
                                   h->w_totals.as<unsigned long long>()));
        HIP_TRY(hipMemcpyAsync(out, h->w_totals.p, sizeof(out), hipMemcpyDeviceToHost, h->stream));
        HIP_TRY(hipStreamSynchronize(h->stream));
    }
    if (h->last_split && h->split_view) {
        uint64_t c2 = 0, s2 = 0;
        if ((rc = ivfhnsw_gpu_last_scan_counts(h->split_view, &c2, &s2)))
            return rc;
        out[0] += c2;
        out[1] += s2;
        (void)hipSetDevice(h->device);
    }
    if (ncodes)
        *ncodes = out[0];
    if (nsegments)
        *nsegments = out[1];
    return IVFHNSW_OK;
}

const char *ivfhnsw_gpu_last_scan_kernel(ivfhnsw_gpu *h) { return h ? h->last_scan_kernel : ""; }

int ivfhnsw_gpu_last_batch_parts(ivfhnsw_gpu *h, uint64_t *first, uint64_t *second)
{
    if (!h)
        return fail(IVFHNSW_ERR_INVALID, "null handle");
    if (first)
        *first = h->last_parts[0];
    if (second)
        *second = h->last_parts[1];
    return IVFHNSW_OK;
}

int ivfhnsw_gpu_memory_bytes(ivfhnsw_gpu *h, uint64_t *bytes)
{
    if (!h || !bytes)
        return fail(IVFHNSW_ERR_INVALID, "null argument");
    uint64_t s = 0;
    h->for_each_devbuf([&](const DevBuf &b) { s += b.bytes; });
    *bytes = s;
    return IVFHNSW_OK;
}
