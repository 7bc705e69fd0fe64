// ivfhnsw::IndexIVF_HNSW over the MI355X C ABI (include/ivf-hnsw/IndexIVF_HNSW.h).
//
// search / search2 / assign / search_batch run on the device; read / write keep the reference's .index format
// (IndexIVF_HNSW.cpp:637-663,758-779); the construction side (add_batch, train_pq) is a plain host
// implementation kept only so that the drivers' cold-start path works at small scale.
#include <ivf-hnsw/IndexIVF_HNSW.h>
#include <ivf-hnsw/IndexIVF_HNSW_Grouping.h>

#include <ivfhnsw_hip.h>

#include <algorithm>
#include <cfloat>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <mutex>
#include <string>
#include <unordered_map>

namespace ivfhnsw {

namespace {

[[noreturn]] void gpu_fail(const char *what)
{
    throw std::runtime_error(std::string(what) + ": " + ivfhnsw_gpu_last_error());
}

// What searchDisk's device re-rank knows about an index: the .bvecs file its device holds ("" = none) and whether
// IVFHNSW_RERANK=device already tried to load one.  Kept beside the object, not in it: drivers compiled against an
// earlier IndexIVF_HNSW.h allocate the object with that header's size, so the class layout must not grow.
struct BaseState {
    std::string path;
    bool auto_tried = false;
};
std::mutex g_base_mu;
std::unordered_map<const void *, BaseState> g_base;

BaseState base_state(const void *ix)
{
    std::lock_guard<std::mutex> lk(g_base_mu);
    auto it = g_base.find(ix);
    return it == g_base.end() ? BaseState() : it->second;
}

void set_base_state(const void *ix, const BaseState &st)
{
    std::lock_guard<std::mutex> lk(g_base_mu);
    if (st.path.empty() && !st.auto_tried)
        g_base.erase(ix);
    else
        g_base[ix] = st;
}

// The finer device state of an index, beside the object for the same reason: which tables a pass
// changed while the lists on the device stayed current, and how often everything went up as a whole.
struct DeviceSide {
    unsigned tables_dirty = 0;
    size_t full_uploads = 0;
    // set_id_filter: the label set, installed on the handle whenever the device copy is made or remade
    bool has_filter = false, filter_deny = false;
    std::vector<uint32_t> filter_labels;
    // set_id_filter_slot: the label set of every slot in use (empty, or IVFHNSW_FILTER_SLOTS entries), installed likewise
    struct SlotSet {
        bool set = false, deny = false;
        std::vector<uint32_t> labels;
    };
    std::vector<SlotSet> slots;
    // set_id_tags: the tag of every label that carries one, installed likewise
    std::unordered_map<uint32_t, uint16_t> tags;
    // set_id_values: the value of every label that has one, installed likewise
    std::unordered_map<uint32_t, uint32_t> values;
};
std::mutex g_side_mu;
std::unordered_map<const void *, DeviceSide> g_side;

size_t shards_wanted() // IVFHNSW_SHARDS=N: N handles, shard r on device r % (devices of the node), lists c % N == r
{
    static const size_t n = [] {
        const char *e = getenv("IVFHNSW_SHARDS");
        const long v = (e && *e) ? atol(e) : 1;
        return (size_t)(v < 1 ? 1 : v > 64 ? 64 : v);
    }();
    return n;
}

// the index's label filter onto its handle (upload_ivf has cleared whatever the handle held)
void install_id_filter(const void *ix, ivfhnsw_gpu *h)
{
    bool has = false, deny = false;
    std::vector<uint32_t> labels;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(ix);
        if (it != g_side.end() && it->second.has_filter) {
            has = true;
            deny = it->second.filter_deny;
            labels = it->second.filter_labels;
        }
    }
    if (has && ivfhnsw_gpu_set_filter(h, labels.size(), labels.data(), deny ? IVFHNSW_FILTER_DENY : IVFHNSW_FILTER_ALLOW))
        gpu_fail("ivfhnsw_gpu_set_filter");
}

// one slot's set, or with slot < 0 every slot's, onto the handle
void install_id_filter_slots(const void *ix, ivfhnsw_gpu *h, int slot = -1)
{
    std::vector<DeviceSide::SlotSet> slots;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(ix);
        if (it != g_side.end())
            slots = it->second.slots;
    }
    for (size_t s = 0; s < slots.size(); s++)
        if (slots[s].set && (slot < 0 || (size_t)slot == s) &&
            ivfhnsw_gpu_set_filter_slot(h, (unsigned)s, slots[s].labels.size(), slots[s].labels.data(),
                                        slots[s].deny ? IVFHNSW_FILTER_DENY : IVFHNSW_FILTER_ALLOW))
            gpu_fail("ivfhnsw_gpu_set_filter_slot");
}

// the index's row tags onto its handle, all of them in one call
void install_id_tags(const void *ix, ivfhnsw_gpu *h)
{
    std::vector<uint32_t> labels;
    std::vector<uint16_t> tags;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(ix);
        if (it != g_side.end())
            for (const auto &lt : it->second.tags) {
                labels.push_back(lt.first);
                tags.push_back(lt.second);
            }
    }
    if (!labels.empty() && ivfhnsw_gpu_set_tags(h, labels.size(), labels.data(), tags.data()))
        gpu_fail("ivfhnsw_gpu_set_tags");
}

// the index's row values onto its handle, all of them in one call
void install_id_values(const void *ix, ivfhnsw_gpu *h)
{
    std::vector<uint32_t> labels, values;
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(ix);
        if (it != g_side.end())
            for (const auto &lv : it->second.values) {
                labels.push_back(lv.first);
                values.push_back(lv.second);
            }
    }
    if (!labels.empty() && ivfhnsw_gpu_set_values(h, labels.size(), labels.data(), values.data()))
        gpu_fail("ivfhnsw_gpu_set_values");
}

// what search_batch (heap_order 1) and range_search (0) ask of the device, for the _slots, _tags, _values and _tags_values forms alike
ivfhnsw_search_params per_query_params(const IndexIVF_HNSW *ix, int heap_order)
{
    const IndexIVF_HNSW_Grouping *grouping = dynamic_cast<const IndexIVF_HNSW_Grouping *>(ix);
    ivfhnsw_search_params p;
    p.nprobe = ix->nprobe;
    p.max_codes = ix->max_codes;
    p.efSearch = ix->quantizer->efSearch;
    p.do_pruning = grouping && grouping->do_pruning ? 1 : 0;
    p.heap_order = heap_order;
    return p;
}

// the results of the range search that just ran on h
void fetch_range_results(ivfhnsw_gpu *h, uint64_t total, std::vector<float> &distances, std::vector<long> &labels)
{
    distances.resize(total);
    labels.resize(total);
    if (ivfhnsw_gpu_range_results(h, 0, total, distances.data(), reinterpret_cast<int64_t *>(labels.data())))
        gpu_fail("ivfhnsw_gpu_range_results");
}

} // namespace

void IndexIVF_HNSW::set_id_filter(size_t n, const idx_t *xids, bool deny)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::set_id_filter: IVFHNSW_SHARDS > 1, and sharded handles have no label filter");
    if (n && !xids)
        throw std::runtime_error("IndexIVF_HNSW::set_id_filter: null ids");
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        DeviceSide &side = g_side[this];
        side.has_filter = true;
        side.filter_deny = deny;
        side.filter_labels.assign(xids, xids + n);
    }
    if (gpu_ && device_current()) // otherwise the next search's upload installs it
        install_id_filter(this, gpu_);
}

void IndexIVF_HNSW::clear_id_filter()
{
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(this);
        if (it != g_side.end()) {
            it->second.has_filter = false;
            std::vector<uint32_t>().swap(it->second.filter_labels);
        }
    }
    if (gpu_ && ivfhnsw_gpu_clear_filter(gpu_))
        gpu_fail("ivfhnsw_gpu_clear_filter");
}

void IndexIVF_HNSW::set_id_filter_slot(unsigned slot, size_t n, const idx_t *xids, bool deny)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::set_id_filter_slot: IVFHNSW_SHARDS > 1, and sharded handles have no filter slots");
    if (slot >= IVFHNSW_FILTER_SLOTS)
        throw std::runtime_error("IndexIVF_HNSW::set_id_filter_slot: slot " + std::to_string(slot) + ", an index has slots 0.." +
                                 std::to_string(IVFHNSW_FILTER_SLOTS - 1));
    if (n && !xids)
        throw std::runtime_error("IndexIVF_HNSW::set_id_filter_slot: null ids");
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        DeviceSide &side = g_side[this];
        side.slots.resize(IVFHNSW_FILTER_SLOTS);
        side.slots[slot].set = true;
        side.slots[slot].deny = deny;
        side.slots[slot].labels.assign(xids, xids + n);
    }
    if (gpu_ && device_current()) // otherwise the next search's upload installs it
        install_id_filter_slots(this, gpu_, (int)slot);
}

void IndexIVF_HNSW::clear_id_filter_slot(int slot)
{
    if (slot < -1 || slot >= IVFHNSW_FILTER_SLOTS)
        throw std::runtime_error("IndexIVF_HNSW::clear_id_filter_slot: slot " + std::to_string(slot));
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(this);
        if (it != g_side.end())
            for (size_t s = 0; s < it->second.slots.size(); s++)
                if (slot < 0 || (size_t)slot == s)
                    it->second.slots[s] = DeviceSide::SlotSet();
    }
    // (a handle without lists holds no slot, and says so)
    if (gpu_ && device_current() && shards_wanted() == 1 && ivfhnsw_gpu_clear_filter_slot(gpu_, slot))
        gpu_fail("ivfhnsw_gpu_clear_filter_slot");
}

void IndexIVF_HNSW::search_batch_slots(size_t nq, size_t k, const float *x, const uint8_t *slots, float *distances,
                                       long *labels)
{
    static_assert(sizeof(long) == sizeof(int64_t), "LP64 expected");
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::search_batch_slots: IVFHNSW_SHARDS > 1, and sharded handles have no filter slots");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 1); // heap order, as search_batch
    if (ivfhnsw_gpu_search_slots(gpu_, nq, k, x, nullptr, nullptr, &p, slots, distances, reinterpret_cast<int64_t *>(labels)))
        gpu_fail("ivfhnsw_gpu_search_slots");
}

void IndexIVF_HNSW::range_search_slots(size_t nq, const float *x, const uint8_t *slots, float radius, std::vector<size_t> &lims,
                                       std::vector<float> &distances, std::vector<long> &labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::range_search_slots: IVFHNSW_SHARDS > 1, and sharded handles have no range search");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 0);
    lims.assign(nq + 1, 0);
    uint64_t total = 0;
    if (ivfhnsw_gpu_range_search_slots(gpu_, nq, x, nullptr, nullptr, &p, slots, radius,
                                       reinterpret_cast<uint64_t *>(lims.data()), &total))
        gpu_fail("ivfhnsw_gpu_range_search_slots");
    fetch_range_results(gpu_, total, distances, labels);
}

void IndexIVF_HNSW::set_id_tags(size_t n, const idx_t *xids, const uint16_t *tags)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::set_id_tags: IVFHNSW_SHARDS > 1, and sharded handles have no row tags");
    if (n && (!xids || !tags))
        throw std::runtime_error("IndexIVF_HNSW::set_id_tags: null ids or tags");
    // an id given two different tags is refused whether or not there is a device copy to refuse it
    std::unordered_map<uint32_t, uint16_t> given;
    for (size_t i = 0; i < n; i++)
        if (!given.emplace(xids[i], tags[i]).second && given[xids[i]] != tags[i])
            throw std::runtime_error("IndexIVF_HNSW::set_id_tags: id " + std::to_string(xids[i]) + " is given two different tags");
    if (gpu_ && device_current() && ivfhnsw_gpu_set_tags(gpu_, n, xids, tags)) // otherwise the next search's upload installs them
        gpu_fail("ivfhnsw_gpu_set_tags");
    std::lock_guard<std::mutex> lk(g_side_mu);
    DeviceSide &side = g_side[this];
    for (const auto &lt : given) {
        if (lt.second == IVFHNSW_TAG_NONE)
            side.tags.erase(lt.first);
        else
            side.tags[lt.first] = lt.second;
    }
}

void IndexIVF_HNSW::clear_id_tags()
{
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(this);
        if (it != g_side.end())
            std::unordered_map<uint32_t, uint16_t>().swap(it->second.tags);
    }
    if (gpu_ && shards_wanted() == 1 && ivfhnsw_gpu_clear_tags(gpu_))
        gpu_fail("ivfhnsw_gpu_clear_tags");
}

void IndexIVF_HNSW::search_batch_tags(size_t nq, size_t k, const float *x, const uint16_t *tags, float *distances, long *labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::search_batch_tags: IVFHNSW_SHARDS > 1, and sharded handles have no row tags");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 1); // heap order, as search_batch
    if (ivfhnsw_gpu_search_tags(gpu_, nq, k, x, nullptr, nullptr, &p, tags, distances, reinterpret_cast<int64_t *>(labels)))
        gpu_fail("ivfhnsw_gpu_search_tags");
}

void IndexIVF_HNSW::range_search_tags(size_t nq, const float *x, const uint16_t *tags, float radius, std::vector<size_t> &lims,
                                      std::vector<float> &distances, std::vector<long> &labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::range_search_tags: IVFHNSW_SHARDS > 1, and sharded handles have no range search");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 0);
    lims.assign(nq + 1, 0);
    uint64_t total = 0;
    if (ivfhnsw_gpu_range_search_tags(gpu_, nq, x, nullptr, nullptr, &p, tags, radius,
                                      reinterpret_cast<uint64_t *>(lims.data()), &total))
        gpu_fail("ivfhnsw_gpu_range_search_tags");
    fetch_range_results(gpu_, total, distances, labels);
}

void IndexIVF_HNSW::set_id_values(size_t n, const idx_t *xids, const uint32_t *values)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::set_id_values: IVFHNSW_SHARDS > 1, and sharded handles have no row values");
    if (n && (!xids || !values))
        throw std::runtime_error("IndexIVF_HNSW::set_id_values: null ids or values");
    // an id given two different values is refused whether or not there is a device copy to refuse it
    std::unordered_map<uint32_t, uint32_t> given;
    for (size_t i = 0; i < n; i++)
        if (!given.emplace(xids[i], values[i]).second && given[xids[i]] != values[i])
            throw std::runtime_error("IndexIVF_HNSW::set_id_values: id " + std::to_string(xids[i]) + " is given two different values");
    if (gpu_ && device_current() && ivfhnsw_gpu_set_values(gpu_, n, xids, values)) // otherwise the next search's upload installs them
        gpu_fail("ivfhnsw_gpu_set_values");
    std::lock_guard<std::mutex> lk(g_side_mu);
    DeviceSide &side = g_side[this];
    for (const auto &lv : given) {
        if (lv.second == IVFHNSW_VALUE_NONE)
            side.values.erase(lv.first);
        else
            side.values[lv.first] = lv.second;
    }
}

void IndexIVF_HNSW::clear_id_values()
{
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        auto it = g_side.find(this);
        if (it != g_side.end())
            std::unordered_map<uint32_t, uint32_t>().swap(it->second.values);
    }
    if (gpu_ && shards_wanted() == 1 && ivfhnsw_gpu_clear_values(gpu_))
        gpu_fail("ivfhnsw_gpu_clear_values");
}

void IndexIVF_HNSW::search_batch_values(size_t nq, size_t k, const float *x, const uint32_t *ranges, float *distances, long *labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::search_batch_values: IVFHNSW_SHARDS > 1, and sharded handles have no row values");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 1); // heap order, as search_batch
    if (ivfhnsw_gpu_search_values(gpu_, nq, k, x, nullptr, nullptr, &p, ranges, distances, reinterpret_cast<int64_t *>(labels)))
        gpu_fail("ivfhnsw_gpu_search_values");
}

void IndexIVF_HNSW::range_search_values(size_t nq, const float *x, const uint32_t *ranges, float radius, std::vector<size_t> &lims,
                                        std::vector<float> &distances, std::vector<long> &labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::range_search_values: IVFHNSW_SHARDS > 1, and sharded handles have no range search");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 0);
    lims.assign(nq + 1, 0);
    uint64_t total = 0;
    if (ivfhnsw_gpu_range_search_values(gpu_, nq, x, nullptr, nullptr, &p, ranges, radius,
                                        reinterpret_cast<uint64_t *>(lims.data()), &total))
        gpu_fail("ivfhnsw_gpu_range_search_values");
    fetch_range_results(gpu_, total, distances, labels);
}

void IndexIVF_HNSW::search_batch_tags_values(size_t nq, size_t k, const float *x, const uint16_t *tags, const uint32_t *ranges,
                                             float *distances, long *labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::search_batch_tags_values: IVFHNSW_SHARDS > 1, and sharded handles have no row tags or values");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 1); // heap order, as search_batch
    if (ivfhnsw_gpu_search_tags_values(gpu_, nq, k, x, nullptr, nullptr, &p, tags, ranges, distances,
                                       reinterpret_cast<int64_t *>(labels)))
        gpu_fail("ivfhnsw_gpu_search_tags_values");
}

void IndexIVF_HNSW::range_search_tags_values(size_t nq, const float *x, const uint16_t *tags, const uint32_t *ranges, float radius,
                                             std::vector<size_t> &lims, std::vector<float> &distances, std::vector<long> &labels)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::range_search_tags_values: IVFHNSW_SHARDS > 1, and sharded handles have no range search");
    ensure_device();
    const ivfhnsw_search_params p = per_query_params(this, 0);
    lims.assign(nq + 1, 0);
    uint64_t total = 0;
    if (ivfhnsw_gpu_range_search_tags_values(gpu_, nq, x, nullptr, nullptr, &p, tags, ranges, radius,
                                             reinterpret_cast<uint64_t *>(lims.data()), &total))
        gpu_fail("ivfhnsw_gpu_range_search_tags_values");
    fetch_range_results(gpu_, total, distances, labels);
}

unsigned IndexIVF_HNSW::tables_dirty() const
{
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto it = g_side.find(this);
    return it == g_side.end() ? 0u : it->second.tables_dirty;
}

void IndexIVF_HNSW::mark_tables_dirty(unsigned which)
{
    std::lock_guard<std::mutex> lk(g_side_mu);
    g_side[this].tables_dirty |= which;
}

size_t IndexIVF_HNSW::device_full_uploads() const
{
    std::lock_guard<std::mutex> lk(g_side_mu);
    auto it = g_side.find(this);
    return it == g_side.end() ? 0 : it->second.full_uploads;
}

IndexIVF_HNSW::IndexIVF_HNSW(size_t dim, size_t ncentroids, size_t bytes_per_code, size_t nbits_per_idx,
                             size_t max_group_size)
    : d(dim), nc(ncentroids), code_size(0), quantizer(nullptr), pq(nullptr), norm_pq(nullptr), opq_matrix(nullptr),
      do_opq(false), nprobe(1), max_codes(0), M(16), gpu_(nullptr), device_dirty_(true), graph_dirty_(true), graph_uploaded_for_(nullptr), latency_for_(nullptr), up_pq_(nullptr),
      up_norm_pq_(nullptr), up_opq_(nullptr), up_quantizer_(nullptr), up_total_(0), up_do_opq_(false)
{
    std::memset(&hdr_idx, 0, sizeof(hdr_idx));
    pq = new faiss::ProductQuantizer(d, bytes_per_code, nbits_per_idx);
    norm_pq = new faiss::ProductQuantizer(1, 1, nbits_per_idx);
    code_size = pq->code_size;
    norms.resize(max_group_size);
    precomputed_table.resize(pq->ksub * pq->M);
    codes.resize(nc);
    norm_codes.resize(nc);
    ids.resize(nc);
    centroid_norms.resize(nc);
}

IndexIVF_HNSW::~IndexIVF_HNSW()
{
    set_base_state(this, BaseState());
    {
        std::lock_guard<std::mutex> lk(g_side_mu);
        g_side.erase(this);
    }
    for (ivfhnsw_gpu *sh : shards_)
        ivfhnsw_gpu_destroy(sh);
    if (gpu_)
        ivfhnsw_gpu_destroy(gpu_);
    delete quantizer;
    delete pq;
    delete norm_pq;
    delete opq_matrix;
}

void IndexIVF_HNSW::build_quantizer(const char *path_data, const char *path_info, const char *path_edges, size_t M_,
                                    size_t efConstruction)
{
    hdr_idx.efConstruction = (uint32_t)efConstruction;
    M = M_;
    device_dirty_ = true;
    graph_dirty_ = true;
    if (exists(path_info) && exists(path_edges)) {
        quantizer = new hnswlib::HierarchicalNSW(path_info, path_data, path_edges);
        quantizer->efSearch = efConstruction;
        return;
    }
    quantizer = new hnswlib::HierarchicalNSW(d, nc, M_, 2 * M_, efConstruction);
    std::cout << "Constructing quantizer\n";
    std::ifstream input(path_data, std::ios::binary);
    // IVFHNSW_BUILD=device: the insertion loop for all centroids at once on the device (ivfhnsw_gpu_build_graph: exact
    // candidates on the matrix cores, then this very heuristic and connect step per node) -- seconds for a million
    // centroids where the serial loop below takes hours (README.md:65 of the reference); the default keeps the serial
    // loop, whose graph equals the reference's link for link.  The device-built graph does NOT: its candidates are the
    // exact nearest earlier centroids, not the results of the reference's greedy search of the graph built so far.  A d
    // the device form does not take (no multiple of 16, as the reference's distance reads it) stays on the serial loop.
    static const bool on_device = [] {
        const char *e = getenv("IVFHNSW_BUILD");
        return e && std::string(e) == "device";
    }();
    if (on_device && nc > 1 && d % 16 == 0 && d <= 128 && 2 * M_ <= 64) {
        std::vector<float> all(nc * d);
        for (size_t i = 0; i < nc; i++)
            readXvec<float>(input, all.data() + i * d, d);
        std::vector<uint8_t> cnt(nc);
        std::vector<idx_t> lk(nc * 2 * M_);
        if (!gpu_ && ivfhnsw_gpu_create(0, &gpu_))
            gpu_fail("ivfhnsw_gpu_create");
        const size_t ncand = std::min<size_t>(80, std::max<size_t>(4 * M_, 2 * M_));
        if (ivfhnsw_gpu_build_graph(gpu_, nc, d, all.data(), M_, 2 * M_, ncand, cnt.data(), lk.data()))
            gpu_fail("ivfhnsw_gpu_build_graph");
        for (size_t i = 0; i < nc; i++) {
            uint8_t *rec = quantizer->get_linklist0((idx_t)i);
            std::memset(rec, 0, quantizer->size_data_per_element);
            rec[0] = cnt[i];
            std::memcpy(rec + 1, lk.data() + i * 2 * M_, (size_t)cnt[i] * sizeof(idx_t));
            std::memcpy(quantizer->getDataByInternalId((idx_t)i), all.data() + i * d, d * sizeof(float));
        }
        quantizer->cur_element_count = nc;
        quantizer->enterpoint_node = 0;
    } else {
        std::vector<float> v(d);
        for (size_t i = 0; i < nc; i++) {
            readXvec<float>(input, v.data(), d);
            if (i % 100000 == 0)
                std::cout << i / (0.01 * nc) << " %\n";
            quantizer->addPoint(v.data());
        }
    }
    quantizer->SaveInfo(path_info);
    quantizer->SaveEdges(path_edges);
}

// ------------------------------------------------------------------------------------------ device mirror
void IndexIVF_HNSW::ensure_latency_walk()
{
    // once per uploaded graph; shapes the latency form does not take (IVFHNSW_ERR_INVALID) keep the throughput walk
    static const bool off = [] {
        const char *e = getenv("IVFHNSW_LATENCY");
        return e && *e && atoi(e) == 0;
    }();
    if (off || latency_for_ == graph_uploaded_for_ || !graph_uploaded_for_)
        return;
    latency_for_ = graph_uploaded_for_;
    const int rc = ivfhnsw_gpu_prepare_latency(gpu_);
    if (rc != IVFHNSW_OK && rc != IVFHNSW_ERR_INVALID)
        gpu_fail("ivfhnsw_gpu_prepare_latency");
}

void IndexIVF_HNSW::ensure_device()
{
    if (!device_current())
        sync_to_device();
    else if (tables_dirty())
        sync_tables_to_device();
}

void IndexIVF_HNSW::sync_tables_to_device()
{
    const unsigned which = tables_dirty();
    if (which & kTableGrouping)
        if (auto *grp = dynamic_cast<IndexIVF_HNSW_Grouping *>(this))
            grp->upload_grouping_tables(); // legal on the lists already there; the lists and the graph stay
    if (which & kTableNorms)
        for (size_t r = 0; r < nshards(); r++)
            if (ivfhnsw_gpu_upload_centroid_norms(shard(r), centroid_norms.data()))
                gpu_fail("ivfhnsw_gpu_upload_centroid_norms");
    std::lock_guard<std::mutex> lk(g_side_mu);
    g_side[this].tables_dirty = 0;
}

bool IndexIVF_HNSW::device_current()
{
    // The list total is the fingerprint that catches a driver appending to the public lists behind the class's back;
    // summing a million list sizes per call would cost more than the search itself (one query per call at 993 127
    // centroids), so beyond 2^16 lists the class relies on its own dirty flags (add_batch, read, invalidate_device()).
    size_t total = up_total_;
    if (nc <= (1u << 16) || !gpu_) {
        total = 0;
        for (size_t c = 0; c < nc; c++)
            total += ids[c].size();
    }
    return gpu_ && !device_dirty_ && up_pq_ == pq && up_norm_pq_ == norm_pq && up_opq_ == opq_matrix &&
           up_quantizer_ == quantizer && up_total_ == total && up_do_opq_ == do_opq;
}

void IndexIVF_HNSW::device_upload_common()
{
    if (!quantizer)
        throw std::runtime_error("IndexIVF_HNSW: no quantizer (call build_quantizer first)");
    if (!gpu_ && ivfhnsw_gpu_create(0, &gpu_))
        gpu_fail("ivfhnsw_gpu_create");
    if (do_opq && !opq_matrix)
        throw std::runtime_error("IndexIVF_HNSW: do_opq is set but opq_matrix is null");
    if (pq->centroids.size() != 256 * d || norm_pq->centroids.size() != 256)
        throw std::runtime_error("IndexIVF_HNSW: pq / norm_pq have unexpected shapes");
    const size_t want_shards = shards_wanted();
    if (nshards() != want_shards) {
        for (ivfhnsw_gpu *sh : shards_)
            ivfhnsw_gpu_destroy(sh);
        shards_.clear();
        int ndev = 1;
        if (ivfhnsw_gpu_device_count(&ndev) || ndev < 1)
            gpu_fail("ivfhnsw_gpu_device_count");
        for (size_t r = 1; r < want_shards; r++) {
            ivfhnsw_gpu *sh = nullptr;
            if (ivfhnsw_gpu_create((int)(r % (size_t)ndev), &sh))
                gpu_fail("ivfhnsw_gpu_create");
            shards_.push_back(sh);
        }
    }
    const size_t world = nshards();

    std::vector<uint64_t> off(nc + 1, 0);
    for (size_t c = 0; c < nc; c++) {
        if (codes[c].size() != ids[c].size() * code_size || norm_codes[c].size() != ids[c].size())
            throw std::runtime_error("IndexIVF_HNSW: list " + std::to_string(c) + " has inconsistent sizes");
        off[c + 1] = off[c] + ids[c].size();
    }
    const size_t total = off[nc];
    for (size_t r = 0; r < world; r++) {
        size_t mine = 0;
        for (size_t c = r; c < nc; c += world)
            mine += ids[c].size();
        std::vector<idx_t> fid(mine ? mine : 1);
        std::vector<uint8_t> fcode(mine ? mine * code_size : 1), fnorm(mine ? mine : 1);
        size_t at = 0;
        for (size_t c = r; c < nc; c += world) { // list order is scan order (ties): keep it
            std::copy(ids[c].begin(), ids[c].end(), fid.begin() + at);
            std::copy(codes[c].begin(), codes[c].end(), fcode.begin() + at * code_size);
            std::copy(norm_codes[c].begin(), norm_codes[c].end(), fnorm.begin() + at);
            at += ids[c].size();
        }
        ivfhnsw_ivf_desc desc;
        std::memset(&desc, 0, sizeof(desc));
        desc.d = d;
        desc.nc = nc;
        desc.code_size = code_size;
        desc.offsets = off.data();
        desc.ids = fid.data();
        desc.codes = fcode.data();
        desc.norm_codes = fnorm.data();
        desc.centroid_norms = centroid_norms.data();
        desc.pq_centroids = pq->centroids.data();
        desc.norm_table = norm_pq->centroids.data();
        desc.opq_A = do_opq ? opq_matrix->A.data() : nullptr;
        desc.shard_rank = (uint32_t)r;
        desc.shard_world = (uint32_t)world;
        desc.list_owner = nullptr;
        if (ivfhnsw_gpu_upload_ivf(shard(r), &desc))
            gpu_fail("ivfhnsw_gpu_upload_ivf");
    }

    upload_graph();
    if (shards_need_graph())
        for (ivfhnsw_gpu *sh : shards_)
            upload_graph_to(sh);

    up_pq_ = pq;
    up_norm_pq_ = norm_pq;
    up_opq_ = opq_matrix;
    up_quantizer_ = quantizer;
    up_total_ = total;
    up_do_opq_ = do_opq;
    if (world == 1) {
        install_id_filter(this, gpu_); // upload_ivf dropped the handle's
        install_id_filter_slots(this, gpu_);
        install_id_tags(this, gpu_);
        install_id_values(this, gpu_);
    }
    std::lock_guard<std::mutex> lk(g_side_mu);
    DeviceSide &side = g_side[this];
    side.tables_dirty = 0;
    side.full_uploads++;
}

void IndexIVF_HNSW::upload_graph()
{
    upload_graph_to(gpu_);
    graph_dirty_ = false;
    graph_uploaded_for_ = quantizer;
    // ivfhnsw_gpu_upload_quantizer discards the fat copy the latency walk reads: the next one-query search() must
    // prepare it again even though the quantizer POINTER is the one it was prepared for (add_batch, read and
    // rotate_quantizer all come through here)
    latency_for_ = nullptr;
}

void IndexIVF_HNSW::upload_graph_to(ivfhnsw_gpu *handle)
{
    // node records [count][maxM links][d floats] -> three arrays
    const size_t maxM = quantizer->maxM_, n = quantizer->maxelements_;
    std::vector<uint8_t> cnt(n);
    std::vector<uint32_t> lnk(n * maxM, 0);
    std::vector<float> vec(n * d);
    for (size_t i = 0; i < n; i++) {
        const uint8_t *rec = quantizer->get_linklist0((idx_t)i);
        cnt[i] = rec[0];
        std::memcpy(&lnk[i * maxM], rec + 1, (size_t)rec[0] * sizeof(uint32_t));
        std::memcpy(&vec[i * d], quantizer->getDataByInternalId((idx_t)i), d * sizeof(float));
    }
    if (ivfhnsw_gpu_upload_quantizer(handle, n, d, maxM, quantizer->enterpoint_node, cnt.data(), lnk.data(), vec.data()))
        gpu_fail("ivfhnsw_gpu_upload_quantizer");
}

void IndexIVF_HNSW::ensure_encoder()
{
    if (!quantizer)
        throw std::runtime_error("IndexIVF_HNSW: no quantizer (call build_quantizer first)");
    if (!pq || !norm_pq)
        throw std::runtime_error("IndexIVF_HNSW::add_batch: pq / norm_pq are not set (train_pq or read them first)");
    if (do_opq && !opq_matrix)
        throw std::runtime_error("IndexIVF_HNSW: do_opq is set but opq_matrix is null");
    if (pq->centroids.size() != 256 * d || norm_pq->centroids.size() != 256)
        throw std::runtime_error("IndexIVF_HNSW: pq / norm_pq have unexpected shapes");
    if (!gpu_ && ivfhnsw_gpu_create(0, &gpu_))
        gpu_fail("ivfhnsw_gpu_create");
    if (graph_dirty_ || graph_uploaded_for_ != quantizer)
        upload_graph();
    // 192 KB: sent with every batch, so a driver that retrains or swaps pq / opq_matrix in place is always seen
    if (ivfhnsw_gpu_upload_codebooks(gpu_, d, code_size, pq->centroids.data(), norm_pq->centroids.data(),
                                     do_opq ? opq_matrix->A.data() : nullptr))
        gpu_fail("ivfhnsw_gpu_upload_codebooks");
}

void IndexIVF_HNSW::sync_to_device()
{
    device_upload_common();
    device_dirty_ = false;
}

// ------------------------------------------------------------------------------------------ search side
void IndexIVF_HNSW::assign(size_t n, const float *x, idx_t *labels, size_t k)
{
    ensure_device();
    std::vector<float> dist(n * k);
    if (ivfhnsw_gpu_coarse(gpu_, n, x, k, quantizer->efSearch < k ? k : quantizer->efSearch, labels, dist.data()))
        gpu_fail("ivfhnsw_gpu_coarse");
}

// Every search of the class: one handle, or -- IVFHNSW_SHARDS=N -- the shard step of SURVEY 8e merged on the host.
// Keys are the library's packed (orderable distance << 32 | scan position) words, sign-flipped so that a signed
// minimum picks the reference's winner (smallest distance, earliest scan position on ties).
namespace {
const uint64_t kSignFlipH = 0x8000000000000000ull;
const uint64_t kKeyInitH = (uint64_t)(0x7f7fffffu | 0x80000000u) << 32;
inline float key_dist(uint64_t ukey)
{
    const uint32_t o = (uint32_t)(ukey >> 32);
    const uint32_t u = (o & 0x80000000u) ? (o & 0x7fffffffu) : ~o;
    float f;
    std::memcpy(&f, &u, sizeof(f));
    return f;
}
inline uint64_t key_pack(float dist, uint32_t vpos)
{
    uint32_t u;
    std::memcpy(&u, &dist, sizeof(u));
    const uint32_t o = (u & 0x80000000u) ? ~u : (u | 0x80000000u);
    return ((uint64_t)o << 32) | vpos;
}
} // namespace

void IndexIVF_HNSW::device_search(size_t nq, size_t k, const float *x, const idx_t *coarse_ids, const float *coarse_dists,
                                  size_t nprobe_, size_t max_codes_, bool pruning, float *distances, long *labels)
{
    static_assert(sizeof(long) == sizeof(int64_t), "LP64 expected");
    ivfhnsw_search_params p;
    p.nprobe = nprobe_;
    p.max_codes = max_codes_;
    p.efSearch = quantizer->efSearch;
    p.do_pruning = pruning ? 1 : 0;
    p.heap_order = 1; // k > 1: the array faiss's max-heap leaves, as the reference returns it
    if (shards_.empty()) {
        if (ivfhnsw_gpu_search(gpu_, nq, k, x, coarse_ids, coarse_dists, &p, distances, reinterpret_cast<int64_t *>(labels)))
            gpu_fail("ivfhnsw_gpu_search");
        return;
    }
    if (nq == 0)
        return;
    // the shard step holds one plan per call: at most 2^17 queries (2^14 in heap order, k > 1), like the unsharded
    // entry point, which slices larger batches itself
    const size_t chunk = k > 1 ? ((size_t)1 << 14) : ((size_t)1 << 17);
    if (nq > chunk) {
        for (size_t q0 = 0; q0 < nq; q0 += chunk)
            device_search(std::min(chunk, nq - q0), k, x + q0 * d, coarse_ids ? coarse_ids + q0 * nprobe_ : nullptr,
                          coarse_dists ? coarse_dists + q0 * nprobe_ : nullptr, nprobe_, max_codes_, pruning,
                          distances + q0 * k, labels + q0 * k);
        return;
    }
    const size_t world = nshards();
    // the coarse stage once, on shard 0 (the rotated query walks the rotated graph, IndexIVF_HNSW.cpp:240,248)
    std::vector<idx_t> cid_own;
    std::vector<float> cd_own;
    if (!coarse_ids) {
        std::vector<float> xr;
        const float *q = x;
        if (do_opq) {
            xr.resize(nq * d);
            opq_matrix->apply_noalloc((long)nq, x, xr.data());
            q = xr.data();
        }
        cid_own.resize(nq * nprobe_);
        cd_own.resize(nq * nprobe_);
        if (ivfhnsw_gpu_coarse(gpu_, nq, q, nprobe_, quantizer->efSearch, cid_own.data(), cd_own.data()))
            gpu_fail("ivfhnsw_gpu_coarse");
        coarse_ids = cid_own.data();
        coarse_dists = cd_own.data();
    }
    const bool heap = k > 1;
    p.heap_order = heap ? 1 : 0;
    if (!heap) {
        // k = 1 (every preset of the reference): the whole shard step below the C ABI -- scans on the shards' devices, the
        // keys MIN-merged and the labels MAX-merged over RCCL between the devices (on the host when shards share a device)
        std::vector<ivfhnsw_gpu *> hs(world);
        for (size_t r = 0; r < world; r++)
            hs[r] = shard(r);
        if (ivfhnsw_gpu_search_sharded(hs.data(), world, nq, k, x, coarse_ids, coarse_dists, &p, distances,
                                       reinterpret_cast<int64_t *>(labels)))
            gpu_fail("ivfhnsw_gpu_search_sharded");
        return;
    }
    std::vector<std::vector<int64_t>> keys(world, std::vector<int64_t>(nq * k));
    std::vector<std::string> err(world);
    // one host thread per shard: every handle has its own device and stream
#pragma omp parallel for schedule(static, 1)
    for (long r = 0; r < (long)world; r++)
        if (ivfhnsw_gpu_search_keys(shard((size_t)r), nq, k, x, coarse_ids, coarse_dists, &p, keys[(size_t)r].data()))
            err[(size_t)r] = ivfhnsw_gpu_last_error();
    for (const auto &e : err)
        if (!e.empty())
            throw std::runtime_error("ivfhnsw_gpu_search_keys: " + e);
    std::vector<int64_t> merged(nq * k);
    if (!heap) {
        // k = 1: the smallest key over the shards
        for (size_t i = 0; i < nq; i++) {
            int64_t m = keys[0][i];
            for (size_t r = 1; r < world; r++)
                m = keys[r][i] < m ? keys[r][i] : m;
            merged[i] = m;
        }
    } else {
        // k > 1, the reference's heap ARRAY (IndexIVF_HNSW.cpp:265,285-288): the shards' candidate streams -- supersets
        // of what faiss's heap admits, each in its scan order -- merged by scan position and replayed through the very
        // maxheap_pop / maxheap_push the reference calls; a code failing `dist < distances[0]` leaves the heap untouched
        std::vector<std::vector<uint32_t>> lens(world, std::vector<uint32_t>(nq));
        uint32_t cap = 0, lmax = 1;
        for (size_t r = 0; r < world; r++) {
            if (ivfhnsw_gpu_last_stream(shard(r), nq, 0, nullptr, lens[r].data(), &cap))
                gpu_fail("ivfhnsw_gpu_last_stream");
            for (uint32_t l : lens[r]) {
                if (l > cap)
                    throw std::runtime_error("IndexIVF_HNSW: candidate stream of a query exceeded the device buffer "
                                             "(k / max_codes too large for heap-array order across shards)");
                lmax = l > lmax ? l : lmax;
            }
        }
        std::vector<std::vector<uint64_t>> streams(world, std::vector<uint64_t>(nq * (size_t)lmax));
        for (size_t r = 0; r < world; r++)
            if (ivfhnsw_gpu_last_stream(shard(r), nq, lmax, streams[r].data(), nullptr, &cap))
                gpu_fail("ivfhnsw_gpu_last_stream");
        std::vector<uint64_t> all;
        std::vector<float> hv(k);
        std::vector<long> hp(k);
        for (size_t i = 0; i < nq; i++) {
            all.clear();
            for (size_t r = 0; r < world; r++)
                all.insert(all.end(), streams[r].begin() + i * lmax, streams[r].begin() + i * lmax + lens[r][i]);
            std::sort(all.begin(), all.end(),
                      [](uint64_t a, uint64_t b) { return (uint32_t)a < (uint32_t)b; }); // scan order
            faiss::maxheap_heapify(k, hv.data(), hp.data());
            for (uint64_t ukey : all) {
                const float dj = key_dist(ukey);
                if (dj < hv[0]) {
                    faiss::maxheap_pop(k, hv.data(), hp.data());
                    faiss::maxheap_push(k, hv.data(), hp.data(), dj, (long)(uint32_t)ukey);
                }
            }
            for (size_t j = 0; j < k; j++)
                merged[i * k + j] =
                    (int64_t)((hp[j] < 0 ? kKeyInitH : key_pack(hv[j], (uint32_t)hp[j])) ^ kSignFlipH);
        }
    }
    // every shard resolves the labels it owns (-1 elsewhere): the maximum is the label
    std::vector<std::vector<long>> lab(world, std::vector<long>(nq * k));
    std::vector<std::vector<float>> dis(world, std::vector<float>(nq * k));
#pragma omp parallel for schedule(static, 1)
    for (long r = 0; r < (long)world; r++)
        if (ivfhnsw_gpu_resolve_keys(shard((size_t)r), nq, k, merged.data(), dis[(size_t)r].data(),
                                     reinterpret_cast<int64_t *>(lab[(size_t)r].data())))
            err[(size_t)r] = ivfhnsw_gpu_last_error();
    for (const auto &e : err)
        if (!e.empty())
            throw std::runtime_error("ivfhnsw_gpu_resolve_keys: " + e);
    for (size_t i = 0; i < nq * k; i++) {
        long l = lab[0][i];
        for (size_t r = 1; r < world; r++)
            l = lab[r][i] > l ? lab[r][i] : l;
        labels[i] = l;
        distances[i] = dis[0][i];
    }
}

void IndexIVF_HNSW::search_batch(size_t nq, size_t k, const float *x, float *distances, long *labels)
{
    ensure_device();
    device_search(nq, k, x, nullptr, nullptr, nprobe, max_codes, false, distances, labels);
}

void IndexIVF_HNSW::range_search(size_t nq, const float *x, float radius, std::vector<size_t> &lims,
                                 std::vector<float> &distances, std::vector<long> &labels)
{
    static_assert(sizeof(long) == sizeof(int64_t) && sizeof(size_t) == sizeof(uint64_t), "LP64 expected");
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::range_search: IVFHNSW_SHARDS > 1, and sharded handles have no range search");
    ensure_device();
    const IndexIVF_HNSW_Grouping *grouping = dynamic_cast<const IndexIVF_HNSW_Grouping *>(this);
    ivfhnsw_search_params p;
    p.nprobe = nprobe;
    p.max_codes = max_codes;
    p.efSearch = quantizer->efSearch;
    p.do_pruning = grouping && grouping->do_pruning ? 1 : 0;
    p.heap_order = 0;
    lims.assign(nq + 1, 0);
    uint64_t total = 0;
    if (ivfhnsw_gpu_range_search(gpu_, nq, x, nullptr, nullptr, &p, radius, reinterpret_cast<uint64_t *>(lims.data()), &total))
        gpu_fail("ivfhnsw_gpu_range_search");
    distances.resize(total);
    labels.resize(total);
    if (ivfhnsw_gpu_range_results(gpu_, 0, total, distances.data(), reinterpret_cast<int64_t *>(labels.data())))
        gpu_fail("ivfhnsw_gpu_range_results");
}

void IndexIVF_HNSW::reconstruct_labels(size_t n, const idx_t *labels, float *x)
{
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::reconstruct_labels: IVFHNSW_SHARDS > 1, and a shard holds only its own lists");
    ensure_device();
    if (ivfhnsw_gpu_reconstruct(gpu_, n, labels, IVFHNSW_RECON_ORIGINAL, x, nullptr))
        gpu_fail("ivfhnsw_gpu_reconstruct");
}

void IndexIVF_HNSW::search_and_reconstruct(size_t k, const float *x, float *distances, long *labels, float *recons)
{
    search_and_reconstruct_batch(1, k, x, distances, labels, recons);
}

void IndexIVF_HNSW::search_and_reconstruct_batch(size_t nq, size_t k, const float *x, float *distances, long *labels,
                                                 float *recons)
{
    static_assert(sizeof(long) == sizeof(int64_t), "LP64 expected");
    if (shards_wanted() > 1)
        throw std::runtime_error("IndexIVF_HNSW::search_and_reconstruct_batch: IVFHNSW_SHARDS > 1, and a shard holds only its own lists");
    ensure_device();
    const IndexIVF_HNSW_Grouping *grouping = dynamic_cast<const IndexIVF_HNSW_Grouping *>(this);
    ivfhnsw_search_params p;
    p.nprobe = nprobe;
    p.max_codes = max_codes;
    p.efSearch = quantizer->efSearch;
    p.do_pruning = grouping && grouping->do_pruning ? 1 : 0;
    p.heap_order = 1; // as search_batch: the array faiss's max-heap leaves
    if (ivfhnsw_gpu_search_reconstruct(gpu_, nq, k, x, nullptr, nullptr, &p, IVFHNSW_RECON_ORIGINAL, distances,
                                       reinterpret_cast<int64_t *>(labels), nullptr, recons))
        gpu_fail("ivfhnsw_gpu_search_reconstruct");
}

// ------------------------------------------------------------------------------------------ searchDisk's re-rank
// The base file in HBM (ivfhnsw_gpu_upload_base): records of uint32 dim + d bytes (utils.cpp:98-105), read in chunks of
// at most 256 MB and handed over as the file image, rows d + 4 bytes apart.  Returns the library's status; file errors
// throw.
int IndexIVF_HNSW::load_base(const char *path_base)
{
    if (!gpu_ && ivfhnsw_gpu_create(0, &gpu_))
        gpu_fail("ivfhnsw_gpu_create");
    FILE *f = fopen(path_base, "rb");
    if (!f)
        throw std::runtime_error(std::string("IndexIVF_HNSW::upload_base: cannot open ") + path_base);
    const size_t rec = sizeof(uint32_t) + d;
    fseek(f, 0, SEEK_END);
    const long size = ftell(f);
    fseek(f, 0, SEEK_SET);
    if (size < 0 || (size_t)size % rec) {
        fclose(f);
        throw std::runtime_error(std::string("IndexIVF_HNSW::upload_base: size of ") + path_base +
                                 " is not a multiple of the record size 4 + d");
    }
    const size_t n = (size_t)size / rec, chunk = std::max<size_t>(1, ((size_t)256 << 20) / rec);
    std::vector<uint8_t> buf(std::min(chunk, n) * rec + 1);
    BaseState st = base_state(this);
    st.path.clear();
    set_base_state(this, st);
    int rc = IVFHNSW_OK;
    for (size_t first = 0; first < n && rc == IVFHNSW_OK; first += chunk) {
        const size_t m = std::min(chunk, n - first);
        if (fread(buf.data(), rec, m, f) != m) {
            fclose(f);
            throw std::runtime_error(std::string("IndexIVF_HNSW::upload_base: short read of ") + path_base);
        }
        for (size_t r = 0; r < m; r++) {
            uint32_t dim;
            std::memcpy(&dim, buf.data() + r * rec, sizeof(dim));
            if (dim != d) {
                fclose(f);
                ivfhnsw_gpu_upload_base(gpu_, 0, d, 0, 0, nullptr, d); // no half-loaded store
                throw std::runtime_error(std::string("IndexIVF_HNSW::upload_base: record ") + std::to_string(first + r) +
                                         " of " + path_base + " has dimension " + std::to_string(dim) + ", not " +
                                         std::to_string(d));
            }
        }
        rc = ivfhnsw_gpu_upload_base(gpu_, n, d, first, m, buf.data() + sizeof(uint32_t), rec);
    }
    fclose(f);
    if (rc == IVFHNSW_OK && n) {
        st.path = path_base;
        set_base_state(this, st);
    }
    return rc;
}

void IndexIVF_HNSW::upload_base(const char *path_base)
{
    if (load_base(path_base) != IVFHNSW_OK)
        gpu_fail("ivfhnsw_gpu_upload_base");
}

void IndexIVF_HNSW::release_base()
{
    BaseState st = base_state(this);
    st.path.clear();
    set_base_state(this, st);
    if (gpu_ && ivfhnsw_gpu_upload_base(gpu_, 0, d, 0, 0, nullptr, d))
        gpu_fail("ivfhnsw_gpu_upload_base");
}

// Does the device hold path_base?  With IVFHNSW_RERANK=device the first call loads it; a store that does not fit in
// HBM (or a d the device form does not take) leaves the host loop in charge.
bool IndexIVF_HNSW::device_base_for(const char *path_base)
{
    BaseState st = base_state(this);
    if (!st.path.empty())
        return st.path == path_base;
    static const bool auto_load = [] {
        const char *e = getenv("IVFHNSW_RERANK");
        return e && std::string(e) == "device";
    }();
    if (!auto_load || st.auto_tried)
        return false;
    st.auto_tried = true;
    set_base_state(this, st);
    const int rc = load_base(path_base);
    if (rc == IVFHNSW_OK)
        return true;
    if (rc != IVFHNSW_ERR_NOMEM && rc != IVFHNSW_ERR_INVALID)
        gpu_fail("ivfhnsw_gpu_upload_base");
    std::fprintf(stderr, "IVFHNSW_RERANK=device: %s not loaded (%s); searchDisk re-ranks from the file\n", path_base,
                 ivfhnsw_gpu_last_error());
    return false;
}

void IndexIVF_HNSW::rerank_candidates(size_t nq, size_t kc, const float *x, const long *cand, size_t k, float *distances,
                                      long *labels, const char *path_base)
{
    if (kc <= 4096 && device_base_for(path_base)) {
        if (ivfhnsw_gpu_rerank(gpu_, nq, kc, x, reinterpret_cast<const int64_t *>(cand), k, distances,
                               reinterpret_cast<int64_t *>(labels)))
            gpu_fail("ivfhnsw_gpu_rerank");
        return;
    }
    // the reference's loop (IndexIVF_HNSW_Grouping.cpp:375-394): one read of the base file per result, cmp's order
    std::vector<SearchInfo_t> ranked;
    for (size_t q = 0; q < nq; q++) {
        ranked.clear();
        for (size_t i = 0; i < kc; i++)
            if (cand[q * kc + i] >= 0) {
                SearchInfo_t s;
                s.label = cand[q * kc + i];
                s.distance = getL2Distance(x + q * d, path_base, d, cand[q * kc + i], base_vec);
                ranked.push_back(s);
            }
        std::sort(ranked.begin(), ranked.end(), cmp);
        for (size_t i = 0; i < k; i++) {
            distances[q * k + i] = i < ranked.size() ? ranked[i].distance : FLT_MAX;
            labels[q * k + i] = i < ranked.size() ? ranked[i].label : -1;
        }
    }
}

void IndexIVF_HNSW::searchDisk_batch(size_t nq, size_t k, const float *x, float *distances, long *labels,
                                     const char *path_base, size_t kc)
{
    if (kc == 0)
        kc = k;
    if (k == 0 || kc < k)
        throw std::invalid_argument("IndexIVF_HNSW::searchDisk_batch: needs 1 <= k <= kc");
    std::vector<float> dc(nq * kc);
    std::vector<long> lc(nq * kc);
    search_batch(nq, kc, x, dc.data(), lc.data());
    rerank_candidates(nq, kc, x, lc.data(), k, distances, labels, path_base);
}

void IndexIVF_HNSW::search(size_t k, const float *x, float *distances, long *labels)
{
#ifdef TRACE_CENTROIDS
    trace_query_centroid_dists.clear();
    trace_centroid_idxs.clear();
#endif
    ensure_device();
    ensure_latency_walk();
    search_batch(1, k, x, distances, labels);
}

void IndexIVF_HNSW::search_debug(size_t k, const float *x, float *distances, long *labels)
{
    // search() plus the coarse-stage report of IndexIVF_HNSW.cpp:343-353: the walk runs once, its result is printed
    // (farthest probe first, as the reference loops) and handed to the scan
    ensure_device();
    std::vector<float> xr(d);
    const float *q = x;
    if (do_opq) {
        opq_matrix->apply_noalloc(1, x, xr.data());
        q = xr.data();
    }
    std::vector<idx_t> cid(nprobe);
    std::vector<float> cd(nprobe);
    if (ivfhnsw_gpu_coarse(gpu_, 1, q, nprobe, quantizer->efSearch, cid.data(), cd.data()))
        gpu_fail("ivfhnsw_gpu_coarse");
    std::cout << "coarse centroids info:" << std::endl;
    for (size_t i = nprobe; i-- > 0;) {
        if (cid[i] >= nc)
            continue; // the walk found fewer than nprobe centroids (undefined in the reference)
        std::cout << "centroid " << cid[i] << " with query distance of " << cd[i] << std::endl;
        std::cout << "group size: " << norm_codes[cid[i]].size() << std::endl;
    }
    device_search(1, k, x, cid.data(), cd.data(), nprobe, max_codes, false, distances, labels);
}

IndexIVF_HNSW::idx_t IndexIVF_HNSW::search_enn(const float *x, float *distances, long *labels)
{
    // nprobe = 1, k = 1, independent of the members (IndexIVF_HNSW.cpp:393-451)
    ensure_device();
    std::vector<float> xr(d);
    const float *q = x;
    if (do_opq) {
        opq_matrix->apply_noalloc(1, x, xr.data());
        q = xr.data();
    }
    idx_t cid = 0;
    float cd = 0.f;
    if (ivfhnsw_gpu_coarse(gpu_, 1, q, 1, quantizer->efSearch ? quantizer->efSearch : 1, &cid, &cd))
        gpu_fail("ivfhnsw_gpu_coarse");
    std::cout << "Get centroid in ENN: " << cid << std::endl;
    device_search(1, 1, x, &cid, &cd, 1, max_codes, false, distances, labels);
    return cid;
}

void IndexIVF_HNSW::search2(size_t k, const float *x, float *distances, long *labels, float *query_centroid_dists,
                            idx_t *centroid_idxs)
{
    ensure_device();
    device_search(1, k, x, centroid_idxs, query_centroid_dists, nprobe, max_codes, false, distances, labels);
}

void IndexIVF_HNSW::search2m(size_t k, const float *x, float *distances[], long *labels[],
                             float *query_centroid_dists, idx_t *centroid_idxs)
{
    // one result heap per probe (the reference's variant is racy; this one is well defined): probe i alone
    ensure_device();
    for (size_t i = 0; i < nprobe; i++)
        device_search(1, k, x, centroid_idxs + i, query_centroid_dists + i, 1, (size_t)-1, false, distances[i], labels[i]);
}

void IndexIVF_HNSW::trace_centroids(size_t idx_q, bool missed)
{
    // the coarse trace lives on the device; fetch it for this query on demand is not wired up
    (void)idx_q;
    (void)missed;
    std::cout << "centroids number " << trace_centroid_idxs.size() << std::endl;
}

float IndexIVF_HNSW::pq_L2sqr(const uint8_t *code)
{
    float result = 0.f;
    for (size_t m = 0; m < code_size; m++)
        result += precomputed_table[pq->ksub * m + code[m]];
    return result;
}

// ------------------------------------------------------------------------------------------ construction side
void IndexIVF_HNSW::compute_residuals(size_t n, const float *x, float *residuals, const idx_t *keys)
{
    for (size_t i = 0; i < n; i++)
        faiss::fvec_madd(d, x + i * d, -1.f, quantizer->getDataByInternalId(keys[i]), residuals + i * d);
}

void IndexIVF_HNSW::reconstruct(size_t n, float *x, const float *decoded_residuals, const idx_t *keys)
{
    for (size_t i = 0; i < n; i++)
        faiss::fvec_madd(d, decoded_residuals + i * d, 1.f, quantizer->getDataByInternalId(keys[i]), x + i * d);
}

void IndexIVF_HNSW::add_batch(size_t n, const float *x, const idx_t *xids, const idx_t *precomputed_idx)
{
    // assign -> residual -> (rotate) -> encode -> decode -> (rotate back) -> reconstruct -> norm -> norm code
    // (the reference's IndexIVF_HNSW.cpp:75-121) is one call on the device; the append loop (:122-131) stays here
    ensure_encoder();
    std::vector<idx_t> idx(n);
    std::vector<uint8_t> xcodes(n * code_size), ncodes(n);
    // A device copy that is current (one handle, no grouping tables, nothing ensure_device would re-upload) takes the
    // batch in place: ivfhnsw_gpu_add appends the codes to the lists in HBM, and neither the lists nor
    // the graph go up again.  Every other case -- the first build before any search included -- marks the copy stale.
    const bool in_place = nshards() == 1 && !dynamic_cast<const IndexIVF_HNSW_Grouping *>(this) && device_current();
    if (in_place) {
        if (ivfhnsw_gpu_add(gpu_, n, x, precomputed_idx, quantizer->efSearch, xids, idx.data(), xcodes.data(),
                            ncodes.data()))
            gpu_fail("ivfhnsw_gpu_add");
    } else if (ivfhnsw_gpu_encode(gpu_, n, x, precomputed_idx, quantizer->efSearch, idx.data(), xcodes.data(),
                                  ncodes.data())) {
        gpu_fail("ivfhnsw_gpu_encode");
    }
    for (size_t i = 0; i < n; i++) {
        const idx_t key = idx[i];
        ids[key].push_back(xids[i]);
        codes[key].insert(codes[key].end(), xcodes.begin() + i * code_size, xcodes.begin() + (i + 1) * code_size);
        norm_codes[key].push_back(ncodes[i]);
    }
    if (in_place)
        up_total_ += n;
    else
        device_dirty_ = true;
}

size_t IndexIVF_HNSW::remove_ids(size_t n, const idx_t *xids)
{
    // A current device copy (one handle, nothing ensure_device would re-upload) shrinks in place: ivfhnsw_gpu_remove_ids
    // compacts the lists in HBM and reports the codes it removed per list, so only those host lists are
    // filtered.  Every other case filters every list on the host and marks the copy stale.
    if (n == 0)
        return 0;
    auto *grouping = dynamic_cast<IndexIVF_HNSW_Grouping *>(this);
    const bool in_place = nshards() == 1 && device_current();
    std::vector<uint32_t> per_list;
    uint64_t dev_removed = 0;
    if (in_place) {
        per_list.assign(nc, 0);
        if (ivfhnsw_gpu_remove_ids(gpu_, n, xids, &dev_removed, per_list.data()))
            gpu_fail("ivfhnsw_gpu_remove_ids");
    }
    std::vector<idx_t> labels(xids, xids + n);
    std::sort(labels.begin(), labels.end());
    labels.erase(std::unique(labels.begin(), labels.end()), labels.end());
    size_t removed = 0;
    for (size_t c = 0; c < nc; c++) {
        if (in_place && per_list[c] == 0)
            continue;
        std::vector<idx_t> &lid = ids[c];
        std::vector<uint8_t> &lcode = codes[c], &lnorm = norm_codes[c];
        // the list's rows sub-group by sub-group (one group of the whole list without Grouping tables)
        std::vector<idx_t> whole(1, (idx_t)lid.size());
        std::vector<idx_t> &groups = grouping && !grouping->subgroup_sizes[c].empty() ? grouping->subgroup_sizes[c] : whole;
        size_t r = 0, w = 0;
        for (idx_t &size : groups) {
            const size_t end = r + size;
            for (; r < end; r++) {
                if (std::binary_search(labels.begin(), labels.end(), lid[r])) {
                    size--;
                    continue;
                }
                lid[w] = lid[r];
                std::copy(lcode.begin() + r * code_size, lcode.begin() + (r + 1) * code_size, lcode.begin() + w * code_size);
                lnorm[w] = lnorm[r];
                w++;
            }
        }
        if (r != lid.size())
            throw std::runtime_error("IndexIVF_HNSW::remove_ids: the sub-group sizes of list " + std::to_string(c) +
                                     " do not add up to its length");
        const size_t gone = r - w;
        if (in_place && gone != per_list[c])
            throw std::runtime_error("IndexIVF_HNSW::remove_ids: list " + std::to_string(c) + " lost " +
                                     std::to_string(gone) + " codes on the host, " + std::to_string(per_list[c]) +
                                     " on the device");
        lid.resize(w);
        lcode.resize(w * code_size);
        lnorm.resize(w);
        removed += gone;
    }
    if (in_place) {
        if (removed != dev_removed)
            throw std::runtime_error("IndexIVF_HNSW::remove_ids: " + std::to_string(removed) + " codes removed on the host, " +
                                     std::to_string(dev_removed) + " on the device");
        up_total_ -= removed;
    } else if (removed) {
        device_dirty_ = true;
    }
    return removed;
}

size_t IndexIVF_HNSW::update_batch(size_t n, const float *x, const idx_t *xids, const idx_t *precomputed_idx)
{
    // remove_ids + add_batch on the host lists; a current device copy (one handle) follows by ONE ivfhnsw_gpu_upsert_ivf
    // with the codes computed here, every other case marks the copy stale.
    if (dynamic_cast<IndexIVF_HNSW_Grouping *>(this))
        throw std::runtime_error("IndexIVF_HNSW_Grouping::update_batch: a Grouping index has no update (the code's sub-group "
                                 "and its group's alpha would have to be derived again); remove_ids, then add_group");
    if (n == 0)
        return 0;
    std::vector<idx_t> labels(xids, xids + n);
    std::sort(labels.begin(), labels.end());
    const auto twice = std::adjacent_find(labels.begin(), labels.end());
    if (twice != labels.end())
        throw std::invalid_argument("IndexIVF_HNSW::update_batch: label " + std::to_string(*twice) + " comes twice in one batch");
    ensure_encoder();
    std::vector<idx_t> idx(n);
    std::vector<uint8_t> xcodes(n * code_size), ncodes(n);
    if (ivfhnsw_gpu_encode(gpu_, n, x, precomputed_idx, quantizer->efSearch, idx.data(), xcodes.data(), ncodes.data()))
        gpu_fail("ivfhnsw_gpu_encode");
    const bool in_place = nshards() == 1 && device_current();
    std::vector<uint32_t> per_list;
    uint64_t dev_removed = 0;
    if (in_place) {
        per_list.assign(nc, 0);
        if (ivfhnsw_gpu_upsert_ivf(gpu_, n, idx.data(), xids, xcodes.data(), ncodes.data(), &dev_removed, per_list.data()))
            gpu_fail("ivfhnsw_gpu_upsert_ivf");
    }
    size_t removed = 0;
    for (size_t c = 0; c < nc; c++) {
        if (in_place && per_list[c] == 0)
            continue;
        std::vector<idx_t> &lid = ids[c];
        std::vector<uint8_t> &lcode = codes[c], &lnorm = norm_codes[c];
        size_t w = 0;
        for (size_t r = 0; r < lid.size(); r++) {
            if (std::binary_search(labels.begin(), labels.end(), lid[r]))
                continue;
            lid[w] = lid[r];
            std::copy(lcode.begin() + r * code_size, lcode.begin() + (r + 1) * code_size, lcode.begin() + w * code_size);
            lnorm[w] = lnorm[r];
            w++;
        }
        const size_t gone = lid.size() - w;
        if (in_place && gone != per_list[c])
            throw std::runtime_error("IndexIVF_HNSW::update_batch: list " + std::to_string(c) + " lost " + std::to_string(gone) +
                                     " codes on the host, " + std::to_string(per_list[c]) + " on the device");
        lid.resize(w);
        lcode.resize(w * code_size);
        lnorm.resize(w);
        removed += gone;
    }
    if (in_place && removed != dev_removed)
        throw std::runtime_error("IndexIVF_HNSW::update_batch: " + std::to_string(removed) + " codes removed on the host, " +
                                 std::to_string(dev_removed) + " on the device");
    for (size_t i = 0; i < n; i++) {
        const idx_t key = idx[i];
        ids[key].push_back(xids[i]);
        codes[key].insert(codes[key].end(), xcodes.begin() + i * code_size, xcodes.begin() + (i + 1) * code_size);
        norm_codes[key].push_back(ncodes[i]);
    }
    if (in_place)
        up_total_ = up_total_ - removed + n;
    else
        device_dirty_ = true;
    return removed;
}

void IndexIVF_HNSW::add_batch2(size_t, const float *, const idx_t *, const idx_t *, uint64_t *, char *)
{
    throw std::runtime_error("IndexIVF_HNSW::add_batch2: the ORCV vendor format is out of scope (SURVEY.md 2, row 9)");
}

void IndexIVF_HNSW::train_pq(size_t n, const float *x)
{
    std::vector<idx_t> assigned(n);
    assign(n, x, assigned.data());
    std::vector<float> res(n * d), tmp;
    compute_residuals(n, x, res.data(), assigned.data());
    if (do_opq) {
        faiss::OPQMatrix *matrix = new faiss::OPQMatrix((int)d, (int)pq->M);
        matrix->verbose = true;
        matrix->max_train_points = n;
        matrix->niter = 70;
        try {
            matrix->train((long)n, res.data());
        } catch (...) {
            delete matrix;
            throw;
        }
        opq_matrix = matrix;
        tmp = res;
        opq_matrix->apply_noalloc((long)n, tmp.data(), res.data());
    }
    printf("Training %zdx%zd product quantizer on %zd vectors in %zdD\n", pq->M, pq->ksub, n, d);
    pq->verbose = true;
    pq->train((int)n, res.data());
    std::vector<uint8_t> xcodes(n * code_size);
    pq->compute_codes(res.data(), xcodes.data(), n);
    std::vector<float> dec(n * d);
    pq->decode(xcodes.data(), dec.data(), n);
    if (do_opq) {
        tmp = dec;
        opq_matrix->transform_transpose((long)n, tmp.data(), dec.data());
    }
    std::vector<float> rec(n * d), nrm(n);
    reconstruct(n, rec.data(), dec.data(), assigned.data());
    faiss::fvec_norms_L2sqr(nrm.data(), rec.data(), d, n);
    printf("Training %zdx%zd product quantizer on %zd vectors in %zdD\n", norm_pq->M, norm_pq->ksub, n, (size_t)1);
    norm_pq->verbose = true;
    norm_pq->train((int)n, nrm.data());
    device_dirty_ = true;
}

int IndexIVF_HNSW::copy_file(const char *file_src, const char *file_dst)
{
    std::ifstream in(file_src, std::ios::binary);
    std::ofstream out(file_dst, std::ios::binary | std::ios::trunc);
    if (!in || !out)
        return -1;
    out << in.rdbuf();
    return out ? 0 : -1;
}

// ------------------------------------------------------------------------------------------ .index files
void IndexIVF_HNSW::write(const char *path_index, bool do_trunc)
{
    std::ofstream out(path_index, do_trunc ? (std::ios::binary | std::ios::trunc) : std::ios::binary);
    write_variable(out, d);
    write_variable(out, nc);
    for (size_t c = 0; c < nc; c++)
        write_vector(out, ids[c]);
    for (size_t c = 0; c < nc; c++)
        write_vector(out, codes[c]);
    for (size_t c = 0; c < nc; c++)
        write_vector(out, norm_codes[c]);
    write_vector(out, centroid_norms);
}

void IndexIVF_HNSW::write(const char *path_index) { this->write(path_index, false); }

void IndexIVF_HNSW::write2(const char *, size_t, bool, const char *)
{
    throw std::runtime_error("IndexIVF_HNSW::write2: the ORCV vendor format is out of scope (SURVEY.md 2, row 9)");
}

void IndexIVF_HNSW::read(const char *path_index)
{
    std::ifstream in(path_index, std::ios::binary);
    if (!in)
        throw std::runtime_error(std::string("cannot open ") + path_index);
    read_variable(in, d);
    read_variable(in, nc);
    ids.resize(nc);
    codes.resize(nc);
    norm_codes.resize(nc);
    for (size_t c = 0; c < nc; c++)
        read_vector(in, ids[c]);
    for (size_t c = 0; c < nc; c++)
        read_vector(in, codes[c]);
    for (size_t c = 0; c < nc; c++)
        read_vector(in, norm_codes[c]);
    read_vector(in, centroid_norms);
    if (!in)
        throw std::runtime_error(std::string("truncated index file ") + path_index);
    device_dirty_ = true;
}

void IndexIVF_HNSW::compute_centroid_norms()
{
    // lists current on the device: a pass that changed no bit dirties nothing, one that did re-sends the norms alone
    const bool current = device_current();
    bool changed = false;
    for (size_t i = 0; i < nc; i++) {
        const float v = faiss::fvec_norm_L2sqr(quantizer->getDataByInternalId((idx_t)i), d);
        changed |= std::memcmp(&v, &centroid_norms[i], sizeof(float)) != 0;
        centroid_norms[i] = v;
    }
    if (!current)
        device_dirty_ = true;
    else if (changed)
        mark_tables_dirty(kTableNorms);
}

void IndexIVF_HNSW::rotate_quantizer()
{
    if (!do_opq) {
        printf("OPQ encoding is turned off\n");
        abort();
    }
    std::vector<float> tmp(d);
    for (size_t i = 0; i < nc; i++) {
        float *c = quantizer->getDataByInternalId((idx_t)i);
        std::memcpy(tmp.data(), c, d * sizeof(float));
        opq_matrix->apply_noalloc(1, tmp.data(), c);
    }
    device_dirty_ = true;
    graph_dirty_ = true;
}

} // namespace ivfhnsw
