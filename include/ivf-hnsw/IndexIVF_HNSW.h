// ivfhnsw::IndexIVF_HNSW -- the reference's IVFADC index class (IndexIVF_HNSW.h:46-190) with its search path on
// an MI355X.  Same public data members, constructor and method signatures and on-disk format, so the
// reference's drivers (tests/*.cpp) compile against this header unchanged.  What differs is behind search():
// the lists are mirrored to HBM as CSR arrays the first time they are needed and every search runs through the
// C ABI of <ivfhnsw_hip.h> (HNSW walk, PQ table, ADC scan and top-k all on the device).  There is no CPU search
// path: without a gfx950 device search() throws.
//
// Extensions (not in the reference): search_batch(), sync_to_device(), invalidate_device(), upload_base(),
// release_base(), searchDisk_batch(), remove_ids(), update_batch(), set_id_filter(), clear_id_filter(), set_id_filter_slot(),
// clear_id_filter_slot(), search_batch_slots(), range_search_slots(), set_id_tags(), clear_id_tags(),
// search_batch_tags(), range_search_tags(), set_id_values(), clear_id_values(), search_batch_values(),
// range_search_values(), search_batch_tags_values(), range_search_tags_values(), range_search(),
// reconstruct_labels(), search_and_reconstruct(), search_and_reconstruct_batch().
#ifndef IVFHNSW_AMD_INDEX_IVF_HNSW_H
#define IVFHNSW_AMD_INDEX_IVF_HNSW_H

#include <cstdio>
#include <fstream>
#include <iostream>
#include <unordered_map>
#include <vector>

#include <faiss/FaissAssert.h>
#include <faiss/Heap.h>
#include <faiss/ProductQuantizer.h>
#include <faiss/VectorTransform.h>
#include <faiss/index_io.h>
#include <faiss/utils.h>

#include <hnswlib/hnswalg.h>

#include "orcv.h"
#include "utils.h"

#define TRACE_CENTROIDS

struct ivfhnsw_gpu; // opaque device handle of <ivfhnsw_hip.h>

namespace ivfhnsw {

struct IndexIVF_HNSW {
    typedef uint32_t idx_t;

    size_t d;         ///< vector dimension
    size_t nc;        ///< number of coarse centroids (= inverted lists)
    size_t code_size; ///< bytes per PQ code

    hnswlib::HierarchicalNSW *quantizer; ///< coarse quantizer graph over the centroids (owned)

    faiss::ProductQuantizer *pq;        ///< residual code books (owned; drivers replace it)
    faiss::ProductQuantizer *norm_pq;   ///< 1 x 256 quantizer of reconstructed norms (owned)
    faiss::LinearTransform *opq_matrix; ///< OPQ rotation (owned) when do_opq
    bool do_opq;

    size_t nprobe;    ///< lists visited per query
    size_t max_codes; ///< stop after the list that brings the scanned codes to this many

    std::vector<std::vector<idx_t>> ids;          ///< per list: vector ids
    std::vector<std::vector<uint8_t>> codes;      ///< per list: PQ codes, code_size bytes each
    std::vector<std::vector<uint8_t>> norm_codes; ///< per list: norm code

    orcvhdr_t hdr_idx;

    std::vector<float> &get_centroid_norms() { return centroid_norms; }

    // per-query coarse trace kept for source compatibility with the debug drivers; filled by search()
    std::vector<float> trace_query_centroid_dists;
    std::vector<idx_t> trace_centroid_idxs;
    void trace_centroids(size_t idx_q, bool missed);

protected:
    std::vector<float> norms;
    std::vector<float> centroid_norms; ///< ||centroid||^2, saved with the index
    int copy_file(const char *file_src, const char *file_dst);
    size_t M;
    float dmatch = 4444.0;
    float dnear = 8888.0;

public:
    explicit IndexIVF_HNSW(size_t dim, size_t ncentroids, size_t bytes_per_code, size_t nbits_per_idx,
                           size_t max_group_size = 65536);
    virtual ~IndexIVF_HNSW();

    /// Load the graph when both files exist, else build it serially from the centroid file and save it.
    void build_quantizer(const char *path_data, const char *path_info, const char *path_edges, size_t M = 16,
                         size_t efConstruction = 500);

    /// labels[i*k .. ] = the k graph vertices nearest to x_i (device HNSW walk at quantizer->efSearch)
    void assign(size_t n, const float *x, idx_t *labels, size_t k = 1);

    /// One query.  distances / labels hold k entries; unfilled slots are FLT_MAX / -1.
    virtual void search(size_t k, const float *x, float *distances, long *labels);
    virtual void search_debug(size_t k, const float *x, float *distances, long *labels);
    virtual idx_t search_enn(const float *x, float *distances, long *labels);

    /// Extension: nq queries in one device pass (what the hardware is for).
    virtual void search_batch(size_t nq, size_t k, const float *x, float *distances, long *labels);
    /// Extension: faiss's range_search for nq queries (ivfhnsw_gpu_range_search).  Every code that
    /// search_batch would score (this object's nprobe, max_codes, quantizer->efSearch; on an IndexIVF_HNSW_Grouping its
    /// sub-groups and do_pruning; set_id_filter honoured) with dist < radius, strictly: query q's results are entries
    /// [lims[q], lims[q + 1]) of distances and labels, in the order the scan loop meets them; lims has nq + 1 entries.
    /// Non-virtual (the class layout and vtable are those of the other extensions).  Throws with IVFHNSW_SHARDS > 1.
    void range_search(size_t nq, const float *x, float radius, std::vector<size_t> &lims, std::vector<float> &distances,
                      std::vector<long> &labels);

    /// Extension: faiss's reconstruct by id (ivfhnsw_gpu_reconstruct): x[i*d ..] = the vector the index
    /// stores for labels[i] -- anchor + decoded code, in the ORIGINAL space (with OPQ: rotated back) -- taken from the
    /// device copy; the lowest row of a label several codes bear; a label no code bears gives d NaNs (0x7fc00000).
    /// On an IndexIVF_HNSW_Grouping the anchor is the code's sub-centroid.  Non-virtual, like range_search.  Throws
    /// with IVFHNSW_SHARDS > 1.
    void reconstruct_labels(size_t n, const idx_t *labels, float *x);
    /// Extension: faiss's search_and_reconstruct (ivfhnsw_gpu_search_reconstruct): search() / search_batch() and, in
    /// recons[(q*k + j)*d ..], the stored vector of result j of query q -- of the code that won, not of the first code
    /// bearing its label; unfilled slots are d NaNs.  Non-virtual.  Throws with IVFHNSW_SHARDS > 1.
    void search_and_reconstruct(size_t k, const float *x, float *distances, long *labels, float *recons);
    void search_and_reconstruct_batch(size_t nq, size_t k, const float *x, float *distances, long *labels, float *recons);

    virtual void add_batch(size_t n, const float *x, const idx_t *xids, const idx_t *precomputed_idx = nullptr);
    /// Extension: remove every code whose id is one of xids[0..n) from the lists (and their sub-groups); returns how many.
    /// With the device copy current (one handle) the lists shrink in HBM as well (ivfhnsw_gpu_remove_ids); otherwise the
    /// next search uploads them again.
    size_t remove_ids(size_t n, const idx_t *xids);
    /// Extension: the labels xids[0..n) have the new vectors x (faiss update_vectors): the lists change as by
    /// remove_ids(n, xids) followed by add_batch(n, x, xids, precomputed_idx); returns how many codes left.  With the
    /// device copy current (one handle) the device lists change by ONE ivfhnsw_gpu_upsert_ivf with the codes computed here;
    /// otherwise the next search uploads them again.  A label twice in xids throws std::invalid_argument before anything
    /// changes.  Non-virtual; an IndexIVF_HNSW_Grouping throws (a code's sub-group and its group's alpha would have to be
    /// derived again).
    size_t update_batch(size_t n, const float *x, const idx_t *xids, const idx_t *precomputed_idx = nullptr);
    /// Extension: faiss's IDSelector.  Every search entry point (search, search_batch, search2, searchDisk,
    /// searchDisk_batch) returns only codes whose id is one of xids[0..n) -- with deny, only codes whose id is none of
    /// them -- as if every other code failed `dist < distances[0]`; unfilled slots hold FLT_MAX / -1.  The set is kept
    /// on the host (beside the object: the class layout does not grow) and installed on the device copy whenever that is
    /// made or remade, at once if it is current (ivfhnsw_gpu_set_filter).  write() is unaffected.
    /// Throws with IVFHNSW_SHARDS > 1 (sharded handles have no filter).
    void set_id_filter(size_t n, const idx_t *xids, bool deny = false);
    void clear_id_filter();
    /// Extension: an IDSelector PER QUERY (ivfhnsw_gpu_set_filter_slot).  An index holds up to 32 id sets
    /// ("slots"), each allow or deny as set_id_filter's; search_batch_slots / range_search_slots take one byte per query
    /// naming the slot that query is filtered by (0xff: by none), and answer each query as search_batch / range_search
    /// would with that slot's set installed by set_id_filter.  A slot that was never set, or was cleared (slot -1: every
    /// slot), passes nothing.  Independent of set_id_filter, and not combined with it: the _slots calls throw while a
    /// set_id_filter filter is installed.  The sets are kept on the host beside the object and installed on the device
    /// copy whenever that is made or remade, at once if it is current.  Non-virtual.  All throw with IVFHNSW_SHARDS > 1.
    void set_id_filter_slot(unsigned slot, size_t n, const idx_t *xids, bool deny = false);
    void clear_id_filter_slot(int slot = -1);
    void search_batch_slots(size_t nq, size_t k, const float *x, const uint8_t *slots, float *distances, long *labels);
    void range_search_slots(size_t nq, const float *x, const uint8_t *slots, float radius, std::vector<size_t> &lims,
                            std::vector<float> &distances, std::vector<long> &labels);
    /// Extension: DISJOINT id sets -- tenant, shard key, collection -- as one 16-bit tag per id (ivfhnsw_gpu_set_tags,
    /// DESIGN.md 3.21).  set_id_tags is incremental: it (over)writes the tags of the ids given (0xffff untags one) and
    /// leaves every other id's alone; an id given two different tags in one call throws.  search_batch_tags /
    /// range_search_tags take one tag per query and answer each query as search_batch / range_search would with
    /// set_id_filter(ids carrying that tag) installed, a query tagged 0xffff as they would with no filter.  Independent of
    /// set_id_filter and the slots, and not combined with them: the _tags calls throw while a set_id_filter filter is
    /// installed.  The tags are kept on the host beside the object and installed on the device copy whenever that is made
    /// or remade, at once if it is current.  Non-virtual.  All throw with IVFHNSW_SHARDS > 1.
    void set_id_tags(size_t n, const idx_t *xids, const uint16_t *tags);
    void clear_id_tags();
    void search_batch_tags(size_t nq, size_t k, const float *x, const uint16_t *tags, float *distances, long *labels);
    void range_search_tags(size_t nq, const float *x, const uint16_t *tags, float radius, std::vector<size_t> &lims,
                           std::vector<float> &distances, std::vector<long> &labels);
    /// Extension: the INTERVAL predicate -- timestamp, price, version, sequence number between a and b -- as one uint32
    /// value per id (ivfhnsw_gpu_set_values).  set_id_values is incremental as set_id_tags is (0xffffffff
    /// un-values an id; an id given two different values in one call throws).  search_batch_values / range_search_values
    /// take one pair per query, ranges[2q] = lo and ranges[2q + 1] = hi, and answer each query as search_batch /
    /// range_search would with set_id_filter(ids whose value lies in [lo, hi]) installed: unsigned, inclusive at both ends,
    /// an id without a value counting as 0xffffffff, so that (0, 0xffffffff) is the unfiltered query and lo > hi finds
    /// nothing.  Independent of set_id_filter, the slots and the tags, and not combined with them: the _values calls throw
    /// while a set_id_filter filter is installed.  The values are kept on the host beside the object and installed on the
    /// device copy whenever that is made or remade, at once if it is current; add_batch, update_batch and remove_ids keep
    /// them.  Non-virtual.  All throw with IVFHNSW_SHARDS > 1.
    void set_id_values(size_t n, const idx_t *xids, const uint32_t *values);
    void clear_id_values();
    void search_batch_values(size_t nq, size_t k, const float *x, const uint32_t *ranges, float *distances, long *labels);
    void range_search_values(size_t nq, const float *x, const uint32_t *ranges, float radius, std::vector<size_t> &lims,
                             std::vector<float> &distances, std::vector<long> &labels);
    /// Extension: a tag AND an interval per query (ivfhnsw_gpu_search_tags_values), on the tags of
    /// set_id_tags and the values of set_id_values the object already keeps: nothing is added to it.  Query q carries
    /// tags[q] and (ranges[2q], ranges[2q + 1]) and is answered as search_batch / range_search would with
    /// set_id_filter(ids tagged tags[q] whose value lies in the interval) installed; tag 0xffff and (0, 0xffffffff) are the
    /// wildcards of the two sides, a null array makes the call the other side's.  Throws while a set_id_filter filter is
    /// installed, and with IVFHNSW_SHARDS > 1.  Non-virtual.
    void search_batch_tags_values(size_t nq, size_t k, const float *x, const uint16_t *tags, const uint32_t *ranges,
                                  float *distances, long *labels);
    void range_search_tags_values(size_t nq, const float *x, const uint16_t *tags, const uint32_t *ranges, float radius,
                                  std::vector<size_t> &lims, std::vector<float> &distances, std::vector<long> &labels);
    virtual void add_batch2(size_t n, const float *x, const idx_t *xids, const idx_t *idx, uint64_t *eids, char *obuf);
    virtual void train_pq(size_t n, const float *x);

    virtual void write(const char *path_index);
    virtual void write(const char *path_index, bool do_trunc);
    virtual void write2(const char *home_dir, size_t n_vecs, bool do_opq, const char *path_edge);
    virtual void read(const char *path);

    void compute_centroid_norms();
    void rotate_quantizer();

    /// coarse stage supplied by the caller (nearest first), as the reference's search2
    void search2(size_t k, const float *x, float *distances, long *labels, float *query_centroid_dists,
                 idx_t *centroid_idxs);
    void search2m(size_t k, const float *x, float *distances[], long *labels[], float *query_centroid_dists,
                  idx_t *centroid_idxs);

    /// Extension: mirror lists, tables and graph to the device now (search() does it lazily).
    virtual void sync_to_device();
    /// Extension: call after mutating ids/codes/norm_codes/pq/... behind the class's back.
    void invalidate_device() { device_dirty_ = true; }
    /// Extension: how often the lists, tables and code books went to the device as a whole (sync_to_device and the
    /// lazy form of it); in-place additions and table re-sends do not count.
    size_t device_full_uploads() const;

    /// Extension: the raw uint8 base vectors of a .bvecs file (the rows searchDisk reads, utils.cpp:98-105) into HBM,
    /// streamed in chunks of at most 256 MB with every record's dim header checked.  searchDisk / searchDisk_batch with
    /// the same path then re-rank on the device.  release_base() frees the copy.
    void upload_base(const char *path_base);
    void release_base();
    /// Extension: searchDisk for nq queries (IndexIVF_HNSW_Grouping.cpp:365-395): search_batch for kc candidates
    /// (kc = 0: k, exactly nq searchDisk calls; larger: "search more, keep k"), then the k best by exact distance
    /// against the base rows -- on the device when upload_base() loaded path_base and kc <= 4096, else from the file.
    void searchDisk_batch(size_t nq, size_t k, const float *x, float *distances, long *labels, const char *path_base,
                          size_t kc = 0);

protected:
    std::vector<float> precomputed_table;
    float pq_L2sqr(const uint8_t *code);

    ivfhnsw_gpu *gpu_;
    bool device_dirty_;
    void ensure_device();
    /// the device copy is what ensure_device would upload (add_batch then appends to it in place)
    bool device_current();
    void device_upload_common();
    /// The finer state beside device_dirty_: the lists on the device are current, but a table pass (compute_centroid_norms,
    /// compute_inter_centroid_dists) changed values; ensure_device re-sends only those tables.
    /// (Kept beside the object, like the re-rank state: the class layout must not grow.)
    enum { kTableNorms = 1, kTableGrouping = 2 };
    unsigned tables_dirty() const;
    void mark_tables_dirty(unsigned which);
    void sync_tables_to_device();
    /// n codes went into the device lists in place (add_batch, Grouping::add_group): the fingerprint follows
    void device_took(size_t n) { up_total_ += n; }
    /// construction side: graph (once per quantizer state) and code books (every call) for ivfhnsw_gpu_encode
    void ensure_encoder();
    void upload_graph();
    bool graph_dirty_;
    const void *graph_uploaded_for_;
    /// one query per call (what search() is): the latency form of the coarse walk, prepared at the first such call
    /// (ivfhnsw_gpu_prepare_latency; IVFHNSW_LATENCY=0 keeps the throughput walk)
    void ensure_latency_walk();
    const void *latency_for_;
    /// IVFHNSW_SHARDS=N: the lists are split list-wise (c % N) over N device handles -- one per GPU of the node, round
    /// robin when there are fewer -- gpu_ being shard 0; every search is the shard step of SURVEY 8e with the merge done
    /// on the host (keys are nq * k * 8 bytes per shard).  shards_ holds handles 1 .. N-1.
    std::vector<ivfhnsw_gpu *> shards_;
    ivfhnsw_gpu *shard(size_t r) const { return r == 0 ? gpu_ : shards_[r - 1]; }
    size_t nshards() const { return shards_.size() + 1; }
    /// every search of the class ends here: one handle, or the sharded step
    void device_search(size_t nq, size_t k, const float *x, const idx_t *coarse_ids, const float *coarse_dists,
                       size_t nprobe_, size_t max_codes_, bool pruning, float *distances, long *labels);
    void upload_graph_to(ivfhnsw_gpu *handle);
    virtual bool shards_need_graph() const { return false; } ///< Grouping: sub-centroid distances on every shard
    /// searchDisk's second half: cand [nq*kc] (-1 = empty) re-ranked by exact distance against path_base, k kept
    void rerank_candidates(size_t nq, size_t kc, const float *x, const long *cand, size_t k, float *distances,
                           long *labels, const char *path_base);
    bool device_base_for(const char *path_base);
    int load_base(const char *path_base);

private:
    void reconstruct(size_t n, float *x, const float *decoded_residuals, const idx_t *keys);
    void compute_residuals(size_t n, const float *x, float *residuals, const idx_t *keys);
    // cheap fingerprint of what was uploaded, to catch drivers swapping public members
    const void *up_pq_, *up_norm_pq_, *up_opq_, *up_quantizer_;
    size_t up_total_;
    bool up_do_opq_;
};

} // namespace ivfhnsw
#endif
