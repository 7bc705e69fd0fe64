/*
 * ivfhnsw_hip.h -- C ABI of the MI355X (gfx950) IVFADC search path.
 *
 * This is the drop-in boundary: the reference (uniio/ivf-hnsw, C++11, CPU only) has no FFI of its
 * own, so every entry point below cites the reference interface it replaces (file:line relative to
 * the reference tree).  The host-side mirror of the reference classes (the headers under include/ivf-hnsw/,
 * ivf-hnsw_amd/csrc/host/) calls nothing but these functions; INTEGRATION.md shows the binding a
 * maintainer of the reference would add.
 *
 * Conventions: plain C, opaque handle, int status (0 = ok, negative = error, message through
 * ivfhnsw_gpu_last_error()), no exceptions cross the boundary, host pointers passed to upload_*
 * are copied and never retained.  There is no CPU fallback: every call fails with
 * IVFHNSW_ERR_HIP when no gfx950 device is usable.
 */
#ifndef IVFHNSW_HIP_H
#define IVFHNSW_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IVFHNSW_OK 0
#define IVFHNSW_ERR_INVALID (-1) /* bad argument / shape mismatch */
#define IVFHNSW_ERR_HIP (-2)     /* HIP runtime error, or no device */
#define IVFHNSW_ERR_STATE (-3)   /* call order: something required was not uploaded */
#define IVFHNSW_ERR_NOMEM (-4)

typedef struct ivfhnsw_gpu ivfhnsw_gpu;

/* Thread-local message of the last failing call on this thread. */
const char *ivfhnsw_gpu_last_error(void);

/* ABI version of this header (bumped on any signature change). */
int ivfhnsw_gpu_abi_version(void);

/* IndexIVF_HNSW::IndexIVF_HNSW / ~IndexIVF_HNSW (IndexIVF_HNSW.cpp:8-32): device-side state of one
 * index.  `device` is the HIP device ordinal. */
int ivfhnsw_gpu_create(int device, ivfhnsw_gpu **out);
/* HIP devices visible to the process (a sharded index puts one handle on each). */
int ivfhnsw_gpu_device_count(int *count);
int ivfhnsw_gpu_destroy(ivfhnsw_gpu *h);

/* A second search context on the SAME device tables: own stream, own per-batch workspace, nothing copied.
 * Batches submitted to the parent and to its views run concurrently (the walk is ALU-bound, the scan HBM-bound:
 * two batches in flight overlap them and fill each other's tails).  The reference's nearest notion is one
 * IndexIVF_HNSW searched from several OpenMP threads, which its member scratch forbids (SURVEY 8b "Threading").
 * The parent must outlive its views and must not upload again while they exist; uploads on a view fail
 * (IVFHNSW_ERR_STATE).  Destroy with ivfhnsw_gpu_destroy. */
int ivfhnsw_gpu_create_view(ivfhnsw_gpu *parent, ivfhnsw_gpu **out);

/* Optional: run on a caller-owned hipStream_t (passed as void*) instead of the handle's own stream. */
int ivfhnsw_gpu_set_stream(ivfhnsw_gpu *h, void *hip_stream);
/* Block until everything queued on the handle's stream has finished.  Also reports (as
 * IVFHNSW_ERR_STATE) a condition a kernel could not represent, e.g. more than 64 exact distance ties
 * at the efSearch boundary of the HNSW walk; the host-pointer entry points check this themselves. */
int ivfhnsw_gpu_sync(ivfhnsw_gpu *h);

/* The inverted lists and the quantizer tables: the data members of IndexIVF_HNSW
 * (IndexIVF_HNSW.h:50-66,81) after read() (IndexIVF_HNSW.cpp:758-779), flattened to CSR.
 * list c occupies [offsets[c], offsets[c+1]) of ids / norm_codes and code_size times that of codes,
 * in list order (the scan order decides ties, IndexIVF_HNSW.cpp:285).
 *
 * Sharding: with shard_world > 1 the arrays ids/codes/norm_codes hold only the lists this
 * shard owns, concatenated in increasing c; offsets is always the global table, so every shard derives
 * the same scan plan.  List c is owned by rank list_owner[c]; with list_owner == NULL by rank
 * c % shard_world.  The owner table lets the caller keep the lists a query probes together on few ranks
 * (a balanced spatial partition of the centroids), so that a query's table is built and staged on those
 * ranks only. */
typedef struct ivfhnsw_ivf_desc {
    size_t d;                    /* IndexIVF_HNSW.h:50 */
    size_t nc;                   /* :51 */
    size_t code_size;            /* :52; multiple of 4 (IndexIVF_HNSW.cpp:805) */
    const uint64_t *offsets;     /* [nc+1] */
    const uint32_t *ids;         /* :64 */
    const uint8_t *codes;        /* :65 */
    const uint8_t *norm_codes;   /* :66 */
    const float *centroid_norms; /* :81, [nc] */
    const float *pq_centroids;   /* pq->centroids, [code_size][256][d/code_size] (:56) */
    const float *norm_table;     /* norm_pq->centroids, [256] (:57) */
    const float *opq_A;          /* opq_matrix->A, [d][d] row major, or NULL when !do_opq (:58-59) */
    uint32_t shard_rank, shard_world; /* 0, 1 for a single GPU */
    const uint32_t *list_owner;  /* [nc] owning rank of every list (< shard_world), or NULL = c % shard_world */
} ivfhnsw_ivf_desc;
int ivfhnsw_gpu_upload_ivf(ivfhnsw_gpu *h, const ivfhnsw_ivf_desc *desc);

/* Same tables, but codes / norm codes are generated on the device (uniform bytes from `seed`) and
 * ids are the running index: the SIFT1B-shaped synthetic corpus of SURVEY 8d for sizes that never
 * exist on the host.  desc->ids/codes/norm_codes are ignored.  With shard_world > 1 the shard receives
 * exactly the bytes and ids its lists have in the unsharded corpus. */
int ivfhnsw_gpu_upload_ivf_synthetic(ivfhnsw_gpu *h, const ivfhnsw_ivf_desc *desc, uint64_t seed);

/* ---- appends to the device lists -------------------------------------------------------------
 *
 * IndexIVF_HNSW::add_batch appends code i to the END of list idx[i], in input order (IndexIVF_HNSW.cpp:122-131): the
 * lists only grow at their ends.  ivfhnsw_gpu_append_ivf does that to the lists the handle holds, in HBM, without a
 * second upload: code i (ids[i], codes[i*code_size ..], norm_codes[i]) goes to the end of list list_idx[i]; codes of
 * one list keep ascending i.  After any sequence of appends the handle's arrays (offsets, local offsets, codes, norm
 * codes, ids, n_local) are byte for byte what upload_ivf of the concatenated lists holds, so searches (labels,
 * distance bits, the max_codes cut, last_scan_counts) are those of that upload.
 *   Sharded handles (shard_world > 1): pass every shard the whole batch.  Each updates the global offsets and keeps
 *   the codes of the lists it owns (the ownership recorded at upload).
 *   Errors leave the tables exactly as they were: list_idx[i] >= nc or n_local + n >= 2^32 - 1 -> IVFHNSW_ERR_INVALID;
 *   allocation failure -> IVFHNSW_ERR_NOMEM; before upload_ivf, on a view, or on a handle with grouping tables (its
 *   lists grow inside, by ivfhnsw_gpu_append_grouping / ivfhnsw_gpu_add_groups below) -> IVFHNSW_ERR_STATE.  n = 0 does
 *   nothing.
 *   The new arrays are built beside the old ones and swapped in: the peak is twice the list bytes.  The graph and
 *   the latency walk's records are not touched.  Like an upload, an append must not run while views of the handle
 *   exist (ivfhnsw_gpu_create_view): they keep the old arrays, which the append frees.  A view created afterwards
 *   sees the new lists.
 * ivfhnsw_gpu_append_ivf_dev: the same on device pointers (list_idx, ids and codes 4-byte aligned) on the handle's
 *   stream; the ids are checked on the device before anything changes.  Returns when the append is done.
 * ivfhnsw_gpu_add: ivfhnsw_gpu_encode followed by the append, the codes never leaving HBM.  Needs upload_codebooks,
 *   upload_quantizer and upload_ivf; code books whose d or code_size differ from the index, or OPQ in one and not
 *   the other -> IVFHNSW_ERR_INVALID, checked before anything is encoded.  ids [n] are the labels of the new codes;
 *   out_idx [n], out_codes [n*code_size], out_norm_codes [n] (each nullable) receive what encode would return.
 * ivfhnsw_gpu_add_dev: the same on device pointers.
 * ivfhnsw_gpu_download_ivf: the handle's global offsets [nc+1] and its local ids [n_local], codes
 *   [n_local*code_size], norm codes [n_local] (each nullable), in the layout upload_ivf takes. */
int ivfhnsw_gpu_append_ivf(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *ids, const uint8_t *codes,
                           const uint8_t *norm_codes);
int ivfhnsw_gpu_append_ivf_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list_idx, const uint32_t *d_ids,
                               const uint8_t *d_codes, const uint8_t *d_norm_codes);
int ivfhnsw_gpu_add(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *precomputed_idx, size_t efSearch,
                    const uint32_t *ids, uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes);
int ivfhnsw_gpu_add_dev(ivfhnsw_gpu *h, size_t n, const float *d_x, const uint32_t *d_precomputed_idx, size_t efSearch,
                        const uint32_t *d_ids, uint32_t *d_out_idx, uint8_t *d_out_codes, uint8_t *d_out_norm_codes);
int ivfhnsw_gpu_download_ivf(ivfhnsw_gpu *h, uint64_t *offsets, uint32_t *ids, uint8_t *codes, uint8_t *norm_codes);

/* ---- removals from the device lists ------------------------------------------------------------
 *
 * faiss's remove_ids for the lists the handle holds, in HBM, without a second upload.  ivfhnsw_gpu_remove_ids removes
 * every code whose id equals one of labels[0..n) from every list that holds one; the codes that remain keep their order
 * in each list.  Any uint32 label is accepted (0xffffffff included); repeated labels count once, labels that match
 * nothing are ignored.  After the call the handle's arrays (offsets, local offsets, codes, norm codes, ids, n_local)
 * are byte for byte what upload_ivf of the remaining lists holds, so searches (labels, distance bits, the max_codes
 * cut, last_scan_counts) are those of that upload.  On a handle with grouping tables each sub-group loses the codes it
 * held: the sub-group sizes are those upload_grouping would get with each size reduced by its removed codes, and what
 * upload_grouping derives from the sizes (the plan's dedupe choice) follows them; alphas, neighbour ids and
 * inter-centroid distances do not change.
 *   n_removed (nullable) receives the number of codes removed, removed_per_list (nullable, [nc]) the number per list.
 *   Errors leave the tables exactly as they were: null labels with n > 0 -> IVFHNSW_ERR_INVALID; allocation failure
 *   (host or device) -> IVFHNSW_ERR_NOMEM; before upload_ivf, on a view, or on a sharded handle (shard_world > 1: a
 *   shard cannot update the global offsets of lists other shards own) -> IVFHNSW_ERR_STATE.  n = 0, or labels that
 *   match nothing: 0 removed, nothing reallocated.
 *   Synchronous on the handle's stream, like an append.  Like an upload, a removal must not run while views of the
 *   handle exist; the handle's own two-part batches pick up the new lists.  A removal ends the validity of the last
 *   search's plan and candidate stream (resolve_keys*, last_stream*).  The graph and the latency walk's records are
 *   not touched.
 *   Memory: the new lists are built beside the old ones and swapped in (the peak is twice the list bytes), plus a
 *   bitmap of the labels over [0, max label] (max label / 8 bytes, at most 512 MB), a removal mask of one bit per code
 *   (n_local / 8 bytes), the labels' staging (4 n bytes, host form) and [nc] counts; the handle keeps these buffers for
 *   the next call until it is destroyed.
 * ivfhnsw_gpu_remove_ids_dev: the same on device pointers (d_labels 4-byte aligned, d_removed_per_list [nc] nullable),
 *   on the handle's stream; returns when the new arrays are in place.
 * ivfhnsw_gpu_download_grouping: the sub-group sizes the handle holds, [nc*nsubc] as upload_grouping takes them; no
 *   grouping tables -> IVFHNSW_ERR_STATE. */
int ivfhnsw_gpu_remove_ids(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, uint64_t *n_removed, uint32_t *removed_per_list);
int ivfhnsw_gpu_remove_ids_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, uint64_t *n_removed,
                               uint32_t *d_removed_per_list);
int ivfhnsw_gpu_download_grouping(ivfhnsw_gpu *h, uint32_t *subgroup_sizes);

/* ---- upserts: replace vectors by label in the device lists -------------------------------------
 *
 * "This label has a new vector" (faiss's IndexIVF::update_vectors) for the lists the handle holds, in HBM, as ONE
 * atomic call.  ivfhnsw_gpu_upsert_ivf removes every code whose id equals one of ids[0..n) from every list that holds
 * one and puts batch code i (ids[i], codes[i*code_size ..], norm_codes[i]) at the end of list list_idx[i]; the codes
 * that remain keep their order, and the batch codes of one list keep ascending i.  After the call the handle's arrays
 * (offsets, local offsets, codes, norm codes, ids, n_local) are byte for byte what ivfhnsw_gpu_remove_ids(h, n, ids)
 * followed by ivfhnsw_gpu_append_ivf(h, n, list_idx, ids, codes, norm_codes) leaves, so searches (labels, distance bits,
 * the max_codes cut, last_scan_counts) are those of upload_ivf of the updated lists.  A label no row bears is a plain
 * insert; a label several rows bear loses all of them and gains one.  Filter, filter slots, row tags and row values are keyed by
 * label and hold for the new rows as after an append or a removal.
 *   n_removed (nullable) receives the number of codes removed, removed_per_list (nullable, [nc]) the number per list.
 *   Unlike the pair of calls it replaces, the call is atomic: every error leaves tables, filter, slots, tags, values and range
 *   results exactly as they were, and all of them are found before the first byte of a new array is written.
 *   list_idx[i] >= nc, a null buffer with n > 0, n_local + n >= 2^32 - 1 (counted before the removal), or THE SAME
 *   LABEL TWICE IN ONE BATCH (found on the device while the label bitmap is built) -> IVFHNSW_ERR_INVALID; allocation
 *   failure -> IVFHNSW_ERR_NOMEM; before upload_ivf, on a view, on a handle with grouping tables or on a sharded handle
 *   (shard_world > 1) -> IVFHNSW_ERR_STATE.  n = 0 does nothing.
 *   Synchronous on the handle's stream.  No views of the handle may exist during the call.  An upsert ends the validity
 *   of the last search's plan and candidate stream (resolve_keys*, last_stream*).  The graph and the latency walk's
 *   records are not touched.
 *   Memory: ONE set of new arrays is built beside the old ones and swapped in (the peak is twice the list bytes, once,
 *   where the pair of calls reaches it twice), plus removal's bitmap and mask and append's staging and sort workspace,
 *   in the buffers the handle keeps for those calls.  Every old row is read once and every new row written once.
 * ivfhnsw_gpu_upsert_ivf_dev: the same on device pointers (list_idx, ids, codes and removed_per_list 4-byte aligned) on
 *   the handle's stream; list ids and labels are checked on the device before anything changes.  Returns when the new
 *   arrays are in place.
 * ivfhnsw_gpu_upsert: ivfhnsw_gpu_encode followed by the upsert, the codes never leaving HBM; to upsert_ivf what
 *   ivfhnsw_gpu_add is to append_ivf, with add's requirements and out_* arrays.  ivfhnsw_gpu_upsert_dev: on device pointers.
 * Not built: upserts on Grouping handles (a code's sub-group and the group's alpha would have to be re-derived) and on
 *   sharded handles; "last one wins" for a label that comes twice; a count of the batch labels that were new. */
int ivfhnsw_gpu_upsert_ivf(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *ids, const uint8_t *codes,
                           const uint8_t *norm_codes, uint64_t *n_removed, uint32_t *removed_per_list);
int ivfhnsw_gpu_upsert_ivf_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list_idx, const uint32_t *d_ids, const uint8_t *d_codes,
                               const uint8_t *d_norm_codes, uint64_t *n_removed, uint32_t *d_removed_per_list);
int ivfhnsw_gpu_upsert(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *precomputed_idx, size_t efSearch,
                       const uint32_t *ids, uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes, uint64_t *n_removed);
int ivfhnsw_gpu_upsert_dev(ivfhnsw_gpu *h, size_t n, const float *d_x, const uint32_t *d_precomputed_idx, size_t efSearch,
                           const uint32_t *d_ids, uint32_t *d_out_idx, uint8_t *d_out_codes, uint8_t *d_out_norm_codes,
                           uint64_t *n_removed);

/* ---- additions to a Grouping index on the device -----------------------------------------------
 *
 * IndexIVF_HNSW_Grouping::add_group lays a group out as nsubc sub-groups end to end (IndexIVF_HNSW_Grouping.cpp:
 * 127-155), so a Grouping list grows at the end of each of its sub-groups, not only at its own end.
 * ivfhnsw_gpu_append_grouping does that to the lists the handle holds, in HBM: code i (ids[i], codes[i*code_size ..],
 * norm_codes[i]) goes to the end of sub-group sub_idx[i] of list list_idx[i]; codes of one sub-group keep ascending i;
 * codes already there keep their order; alpha, neighbours and inter-centroid distances of the group do not change.
 * After any sequence of calls the handle's arrays (offsets, local offsets, codes, norm codes, ids, n_local, sub-group
 * sizes, and the dedupe choice upload_grouping derives from them) are byte for byte what upload_ivf + upload_grouping
 * of the merged lists hold, so searches (labels, distance bits, the max_codes cut, pruning decisions,
 * last_scan_counts) are those of that upload.
 * ivfhnsw_gpu_add_groups is add_group (:43-157) for groups that hold no codes (never added, or emptied by
 * ivfhnsw_gpu_remove_ids; the vector-add driver's flow, tests/test_ivfhnsw_grouping_sift1b_vector_add.cpp):
 * ivfhnsw_gpu_encode_groups on the same arguments with the handle's nsubc, then for every group with points its
 * nn_centroid_idxs row, its alpha, its inter-centroid-distance row and its codes (sub-group by sub-group, arrival
 * order inside each, :127-155) are installed, the codes never leaving HBM between the encode and the install.  A group
 * with zero points gets its neighbour row and nothing else (:63-64).  ids [offsets[ngroups]] are the labels of the
 * points.  inter_centroid_dists NULL: the rows are computed on the device as compute_inter_centroid_dists does
 * (:620-631); non-NULL ([ngroups*nsubc]): the caller's rows are stored as given.  out_nn_centroid_idxs
 * [ngroups*nsubc], out_alphas [ngroups] (an empty group keeps the caller's value), out_subcentroid_idxs [n], out_codes
 * [n*code_size] and out_norm_codes [n] (nullable) receive what encode_groups returns.
 *   Sharded handles (shard_world > 1): pass every shard the whole batch.  Each updates the global offsets and the
 *   (replicated) grouping tables and keeps the codes of the lists it owns.
 *   Errors are found before anything is written and leave every table exactly as it was: list_idx[i] >= nc,
 *   sub_idx[i] >= nsubc, centroid_idx[g] >= nc, the same centroid twice in one add_groups call, n_local + n >=
 *   2^32 - 1, code books that do not match the index -> IVFHNSW_ERR_INVALID; an add_groups centroid whose list already
 *   holds codes (with or without points of its own in the call) -> IVFHNSW_ERR_STATE, the message naming the list;
 *   before upload_ivf, on a view, or on a handle WITHOUT grouping tables -> IVFHNSW_ERR_STATE; allocation failure ->
 *   IVFHNSW_ERR_NOMEM.  n = 0 / ngroups = 0 does nothing.  (An error of the encode itself -- efSearch < nsubc + 1, a
 *   walk that finds fewer than nsubc + 1 centroids -- also leaves the tables; the out_* arrays may be partly written.)
 *   Views, streams, memory, validity: as for ivfhnsw_gpu_append_ivf (no views alive during the call; synchronous on the
 *   handle's stream; new arrays built beside the old ones and swapped in, peak twice the list bytes, plus three
 *   [nc*nsubc] uint32 work tables the handle keeps) and as for ivfhnsw_gpu_remove_ids (the last search's plan and
 *   candidate stream stop being valid; the graph and the latency walk's records are not touched).
 * The _dev forms: the same on device pointers (4-byte aligned; offsets 8-byte; else IVFHNSW_ERR_INVALID) on the handle's
 *   stream; the ids are checked on the device and a status word read before anything changes.  add_groups_dev reads d_centroid_idx and
 *   d_offsets back first (they steer the chunking of the encode).
 * ivfhnsw_gpu_download_grouping_tables: alphas [nc], nn_centroid_idxs, subgroup_sizes, inter_centroid_dists
 *   [nc*nsubc each] as the handle holds them (each nullable); no grouping tables -> IVFHNSW_ERR_STATE.
 * ivfhnsw_gpu_upload_centroid_norms: replaces the [nc] centroid norms upload_ivf's descriptor brought
 *   (IndexIVF_HNSW::compute_centroid_norms, IndexIVF_HNSW.cpp:930-935) and nothing else; before upload_ivf or on a
 *   view -> IVFHNSW_ERR_STATE. */
int ivfhnsw_gpu_append_grouping(ivfhnsw_gpu *h, size_t n, const uint32_t *list_idx, const uint32_t *sub_idx,
                                const uint32_t *ids, const uint8_t *codes, const uint8_t *norm_codes);
int ivfhnsw_gpu_append_grouping_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_list_idx, const uint32_t *d_sub_idx,
                                    const uint32_t *d_ids, const uint8_t *d_codes, const uint8_t *d_norm_codes);
int ivfhnsw_gpu_add_groups(ivfhnsw_gpu *h, size_t ngroups, const uint32_t *centroid_idx, const uint64_t *offsets, const float *x,
                           size_t efSearch, const uint32_t *ids, const float *inter_centroid_dists,
                           uint32_t *out_nn_centroid_idxs, float *out_alphas, uint32_t *out_subcentroid_idxs, uint8_t *out_codes,
                           uint8_t *out_norm_codes);
int ivfhnsw_gpu_add_groups_dev(ivfhnsw_gpu *h, size_t ngroups, const uint32_t *d_centroid_idx, const uint64_t *d_offsets,
                               const float *d_x, size_t efSearch, const uint32_t *d_ids, const float *d_inter_centroid_dists,
                               uint32_t *d_out_nn_centroid_idxs, float *d_out_alphas, uint32_t *d_out_subcentroid_idxs,
                               uint8_t *d_out_codes, uint8_t *d_out_norm_codes);
int ivfhnsw_gpu_download_grouping_tables(ivfhnsw_gpu *h, float *alphas, uint32_t *nn_centroid_idxs, uint32_t *subgroup_sizes,
                                         float *inter_centroid_dists);
int ivfhnsw_gpu_upload_centroid_norms(ivfhnsw_gpu *h, const float *centroid_norms);

/* Label filter: faiss's IDSelector for the lists the handle holds.  A handle holds no filter or one: a
 * set of uint32 labels and a mode.  IVFHNSW_FILTER_ALLOW: only rows whose id is in the set pass; IVFHNSW_FILTER_DENY:
 * rows whose id is in the set do not pass (soft deletes, without the compaction of ivfhnsw_gpu_remove_ids).  With a
 * filter installed every search on the handle (search, search_dev, search_keys / out_keys; unsharded handles) behaves as
 * the reference's would if a non-passing code failed `dist < distances[0]`: the same lists and sub-groups are visited in
 * the same order, max_codes and Grouping's pruning count every stored code, ivfhnsw_gpu_last_scan_counts and the scan
 * positions in keys and candidate streams are those of the unfiltered call (resolve_keys, last_stream and replay_stream
 * work unchanged); results hold passing labels only, unfilled slots FLT_MAX / -1, and heap_order = 1 leaves the heap
 * array faiss would leave had it seen only the passing codes (any k).  ivfhnsw_gpu_last_scan_kernel reports the
 * filtered launch as the unfiltered name with "+filter" appended; small batches run plan, table and scan instead of the
 * one-launch tail.  Without a filter nothing changes: the same kernels, the same bits.
 *   Any label value is accepted (0xffffffff included); repeated labels count once; labels that match nothing are
 *   ignored; an empty allow set passes nothing, an empty deny set everything.
 * ivfhnsw_gpu_set_filter replaces an earlier filter; the new one is built beside it, so any error leaves the earlier
 *   filter in force.  Synchronous; ~1 bit per label value up to the largest label (<= 512 MB) plus 1 bit per resident
 *   row stay allocated, both counted by ivfhnsw_gpu_memory_bytes.  ivfhnsw_gpu_set_filter_dev: d_labels in device memory
 *   (4-byte aligned), read on the handle's stream; returns with that stream drained.
 * ivfhnsw_gpu_clear_filter: no filter afterwards; succeeds on a handle that has none.  ivfhnsw_gpu_upload_ivf clears it.
 * After a successful append_ivf, add, remove_ids, append_grouping or add_groups (host or _dev form) the filter holds for
 *   the updated lists (rows are judged again from the kept label set); an update that fails leaves tables and filter
 *   as they were.
 * Views: set_filter / clear_filter on a view -> IVFHNSW_ERR_STATE.  A view filters with what its parent held when the
 *   view was created (the internal view of split batches: at every call); replacing or clearing the parent's filter
 *   while a view of it is in use is, like an update of the tables, the caller's to avoid.
 * ivfhnsw_gpu_filter_info: *mode = the installed mode or -1; *rows_passing = resident rows that pass (all of them
 *   without a filter); *rows_total = resident rows.  Each pointer nullable.
 * Errors: before upload_ivf, on a view, on a handle with shard_world > 1 -> IVFHNSW_ERR_STATE; null labels with n > 0
 *   or an unknown mode -> IVFHNSW_ERR_INVALID; a failed allocation -> IVFHNSW_ERR_NOMEM. */
#define IVFHNSW_FILTER_ALLOW 0
#define IVFHNSW_FILTER_DENY 1
int ivfhnsw_gpu_set_filter(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode);
int ivfhnsw_gpu_set_filter_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int mode);
int ivfhnsw_gpu_clear_filter(ivfhnsw_gpu *h);
int ivfhnsw_gpu_filter_info(ivfhnsw_gpu *h, int *mode, uint64_t *rows_passing, uint64_t *rows_total);

/* Filter slots: a label filter PER QUERY.  Beside its one filter a handle holds up to
 * IVFHNSW_FILTER_SLOTS label sets, each a set of uint32 labels and a mode exactly as ivfhnsw_gpu_set_filter takes them
 * (any label value, repeats count once, an empty allow set passes nothing, an empty deny set everything).  A slot that
 * was never set, or was cleared, passes nothing.  The _slots forms of search and range search take one byte per query:
 * query q with query_slots[q] == s answers, bit for bit, what the plain call answers on the same handle with
 * ivfhnsw_gpu_set_filter(labels of s, mode of s) installed -- labels, distance bits, unfilled places FLT_MAX / -1, the
 * heap array of heap_order = 1 (any k), out_keys, candidate streams, resolve_keys*, range lims / distances / labels in
 * scan order -- and with IVFHNSW_SLOT_NONE what it answers with no filter installed.  Everything said above about a
 * filtered call holds per query: the same lists and sub-groups in the same order, max_codes and pruning count every
 * stored code, ivfhnsw_gpu_last_scan_counts is the unfiltered call's.  ivfhnsw_gpu_last_scan_kernel reports the
 * unfiltered name with "+slots" appended; a _slots call runs plan, table and scan (never the one-launch tail or the
 * pipelined scan), large batches split in two parts as plain ones do.  query_slots == NULL is the plain call.
 *   Slots and the handle's filter are independent state: plain calls never read slots, and a _slots call on a handle
 *   that has a set_filter filter installed -> IVFHNSW_ERR_STATE (the two are not combined).
 * ivfhnsw_gpu_set_filter_slot replaces the slot's earlier set; the new one is built beside the installed state, so any
 *   error leaves every slot as it was.  Synchronous on the handle's stream.  _dev: d_labels in device memory (4-byte
 *   aligned).  ivfhnsw_gpu_clear_filter_slot: slot -1 = every slot; succeeds on a slot that is not set.
 *   ivfhnsw_gpu_upload_ivf clears every slot.  ivfhnsw_gpu_filter_slot_info: *mode = the slot's mode or -1,
 *   *rows_passing = resident rows that pass it (0 for a slot that is not set), *rows_total = resident rows; each nullable.
 * Query slot bytes: the host forms check them before anything is launched or written, a byte in 32..254 ->
 *   IVFHNSW_ERR_INVALID.  The _dev forms read nothing back: any byte other than 0xff that names no installed slot passes
 *   nothing (the kernels check the byte against the planes the handle holds).
 * After a successful append_ivf, add, remove_ids, append_grouping or add_groups every installed slot holds for the
 *   updated lists (all slots are judged again in one pass over the new ids); an update that fails leaves tables and
 *   slots as they were.  A view reads the slots its parent held when the view was created (the internal view of split
 *   batches: at every call); set / clear on a view -> IVFHNSW_ERR_STATE.
 * Memory, all counted by ivfhnsw_gpu_memory_bytes: (highest slot in use + 1) planes of 8 * max(ceil(rows / 64), 1)
 *   bytes -- one pass bit per resident row and plane -- plus, per slot with a non-empty set, 4 * (max label / 32 + 1)
 *   bytes of label bitmap (<= 512 MB), kept so that updates can judge new rows.
 * Errors: slot >= IVFHNSW_FILTER_SLOTS, an unknown mode, null labels with n > 0, a misaligned d_labels ->
 *   IVFHNSW_ERR_INVALID; set or clear before upload_ivf, on a view, on a handle with shard_world > 1 -> IVFHNSW_ERR_STATE;
 *   a _slots call on a sharded handle -> IVFHNSW_ERR_STATE; a failed allocation -> IVFHNSW_ERR_NOMEM; whatever the plain
 *   call refuses for the same arguments is refused with its status.
 * Not built: a slot AND the handle's filter; slots for search_reconstruct, search_sharded, and sharded handles; more than
 *   32 slots.  (The exact calls have slots of their own: "base filter slots" below.) */
#define IVFHNSW_FILTER_SLOTS 32
#define IVFHNSW_SLOT_NONE 0xff
int ivfhnsw_gpu_set_filter_slot(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *labels, int mode);
int ivfhnsw_gpu_set_filter_slot_dev(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *d_labels, int mode);
int ivfhnsw_gpu_clear_filter_slot(ivfhnsw_gpu *h, int slot); /* -1: every slot */
int ivfhnsw_gpu_filter_slot_info(ivfhnsw_gpu *h, unsigned slot, int *mode, uint64_t *rows_passing, uint64_t *rows_total);

/* Row tags: DISJOINT sets -- tenant, shard key, collection -- as one 16-bit number per row rather than
 * a bit plane per set: 2 bytes per resident row serve 65 535 sets.  A handle holds at most one tag table, a uint16 per
 * label value over [0, largest label ever tagged]; a label that was never tagged reads as IVFHNSW_TAG_NONE.  The _tags
 * forms of search and range search take one uint16 per query: query q with query_tags[q] == t, t != IVFHNSW_TAG_NONE,
 * answers, bit for bit, what the plain call answers on the same handle with set_filter({labels tagged t}, ALLOW)
 * installed -- labels, distance bits, unfilled places, the heap array of heap_order = 1 for any k, out_keys, candidate
 * streams, resolve_keys*, and range lims / distances / labels in scan order -- and with IVFHNSW_TAG_NONE what it answers
 * with no filter.  Everything said of a filtered call above holds per query (the same lists in the same order,
 * max_codes counts every stored code, last_scan_counts is the unfiltered call's).  A tag that no row carries returns
 * padding / empty lims.  A _tags launch reports the unfiltered kernel's name with "+tags" appended and runs plan, table
 * and scan as a _slots launch does.  query_tags == NULL is the plain call.
 *   Tags, slots and the handle's filter are independent state: plain and _slots calls never read tags, a _tags call
 * ignores slots, and a _tags call on a handle with a set_filter filter installed -> IVFHNSW_ERR_STATE.  A _tags call on a
 * handle without a tag table is legal: every row is IVFHNSW_TAG_NONE.
 * ivfhnsw_gpu_set_tags is INCREMENTAL: it (over)writes the tags of the n labels given and leaves every other label's
 *   alone.  Any uint32 label, resident or not; a repeated label with the same tag counts once; a label given two
 *   different tags in one call -> IVFHNSW_ERR_INVALID; the tag IVFHNSW_TAG_NONE untags a label.  The new table and row
 *   tags are built beside the installed ones and swapped in: any error leaves the state as it was.  Synchronous on the
 *   handle's stream.  _dev: d_labels (4-byte aligned) and d_tags (2-byte aligned) in device memory.
 *   ivfhnsw_gpu_clear_tags drops table and row tags (succeeds without any); ivfhnsw_gpu_upload_ivf does the same.
 *   ivfhnsw_gpu_tags_info: *rows_tagged = resident rows whose tag is not IVFHNSW_TAG_NONE, *rows_total = resident rows,
 *   *table_labels = label values the table spans (largest tagged label + 1; 0 without a table); each nullable.
 *   ivfhnsw_gpu_tag_rows: *rows = resident rows that carry `tag` (tag <= 0xffff; IVFHNSW_TAG_NONE counts the untagged).
 * After a successful append_ivf, add, remove_ids, append_grouping or add_groups (host and _dev forms) the row tags hold
 *   for the updated lists (one gather over the new ids, before they are installed); an update that fails leaves tables and
 *   tags as they were.  A label held by several rows tags all of them.  A view reads the tags its parent held when the view
 *   was created (the internal view of a split batch follows the handle at every call); set / clear on a view ->
 *   IVFHNSW_ERR_STATE.
 * Memory, counted by ivfhnsw_gpu_memory_bytes: 2 * (largest tagged label + 1) bytes of table and 2 * max(rows, 1) bytes of
 *   row tags; a host _tags call stages its 2 bytes per query.
 * Errors: null labels or tags with n > 0, a misaligned device pointer, conflicting repeats, tag > 0xffff ->
 *   IVFHNSW_ERR_INVALID; set before upload_ivf, set or clear on a view, set / clear / a _tags call on a handle with
 *   shard_world > 1 -> IVFHNSW_ERR_STATE; a failed allocation -> IVFHNSW_ERR_NOMEM.
 * The truth of a _tags search: ivfhnsw_gpu_exact_search_tags on a store tagged with ivfhnsw_gpu_set_base_tags ("Base
 *   tags" below), one call for any number of tags.
 * A tag AND a value interval per query: the _tags_values calls ("Row tags AND row values" below).
 * Not built: tags for search_reconstruct, search_sharded and sharded handles; a tag AND the handle's filter or a slot;
 *   tags wider than 16 bits or several tags per row. */
#define IVFHNSW_TAG_NONE 0xffffu
int ivfhnsw_gpu_set_tags(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, const uint16_t *tags);
int ivfhnsw_gpu_set_tags_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, const uint16_t *d_tags);
int ivfhnsw_gpu_clear_tags(ivfhnsw_gpu *h);
int ivfhnsw_gpu_tags_info(ivfhnsw_gpu *h, uint64_t *rows_tagged, uint64_t *rows_total, uint64_t *table_labels);
int ivfhnsw_gpu_tag_rows(ivfhnsw_gpu *h, unsigned tag, uint64_t *rows);

/* Row values: the INTERVAL predicate -- timestamp, price, version, sequence number between a and b --
 * beside the set-membership ones above.  A handle holds at most one value table, a uint32 per label value over [0, largest
 * label ever given a value]; a label that was never given one reads as IVFHNSW_VALUE_NONE.  The _values forms of search
 * and range search take one pair per query: query_ranges [2 * nq] uint32, query q carrying (lo, hi) = (query_ranges[2q],
 * query_ranges[2q + 1]).
 *   The rule: a row passes query q iff lo <= value(row) <= hi, UNSIGNED and INCLUSIVE at both ends.  A row without a value
 * has the value 0xffffffff.  There is deliberately no special case: (0, 0xffffffff) passes every row and is the unfiltered
 * query; (x, 0xfffffffe) is "at least x, among the rows that have a value", (x, 0xffffffff) also admits the rows without
 * one; lo > hi is legal and passes no row -- the query returns padding (FLT_MAX / -1) or an empty range.
 *   Query q answers, bit for bit, what the plain call answers on the same handle with set_filter({labels whose value lies
 * in [lo, hi]}, ALLOW) installed -- labels, distance bits, unfilled places, the heap array of heap_order = 1 for any k
 * (k > 1024 included), out_keys, candidate streams, resolve_keys*, and range lims / distances / labels in scan order --
 * and with (0, 0xffffffff) what it answers with no filter.  Everything said of a filtered call above holds per query (the
 * same lists in the same order, max_codes and Grouping's pruning count every stored code, last_scan_counts is the
 * unfiltered call's).  A _values launch reports the unfiltered kernel's name with "+values" appended and runs plan, table
 * and scan as a _tags launch does.  query_ranges == NULL is the plain call.
 *   Values are a fourth independent state beside filter, slots and tags: plain, _slots and _tags calls never read them, a
 * _values call ignores slots and tags, and a _values call on a handle with a set_filter filter installed ->
 * IVFHNSW_ERR_STATE.  A _values call on a handle without a value table is legal: every row is IVFHNSW_VALUE_NONE.
 * ivfhnsw_gpu_set_values is INCREMENTAL, exactly as set_tags is: it (over)writes the values of the n labels given and
 *   leaves every other label's alone.  Any uint32 label, resident or not; a repeated label with the same value counts
 *   once; a label given two different values in one call -> IVFHNSW_ERR_INVALID; the value IVFHNSW_VALUE_NONE un-values a
 *   label.  The new table and row values are built beside the installed ones and swapped in: any error leaves the state
 *   as it was.  Synchronous on the handle's stream.  _dev: d_labels and d_values in device memory, 4-byte aligned.
 *   ivfhnsw_gpu_clear_values drops table and row values (succeeds without any); ivfhnsw_gpu_upload_ivf does the same.
 *   ivfhnsw_gpu_values_info: *rows_valued = resident rows whose value is not IVFHNSW_VALUE_NONE, *rows_total = resident
 *   rows, *table_labels = label values the table spans (largest valued label + 1; 0 without a table); each nullable.
 *   ivfhnsw_gpu_value_rows: *rows = resident rows an interval passes under the rule above (size max_codes from it).
 * After a successful append_ivf, add, remove_ids, upsert_ivf, upsert, append_grouping or add_groups (host and _dev forms)
 *   the row values hold for the updated lists (one gather over the new ids, before they are installed); an update that
 *   fails leaves lists, filter, slots, tags and values as they were.  A label held by several rows gives all of them its
 *   value.  A view reads the values its parent held when the view was created (the internal view of a split batch follows
 *   the handle at every call); set / clear on a view -> IVFHNSW_ERR_STATE.
 * Memory, counted by ivfhnsw_gpu_memory_bytes: 4 * (largest valued label + 1) bytes of table and 4 * max(rows, 1) bytes
 *   of row values; a host _values call stages its 8 bytes per query.
 * Errors: null labels or values with n > 0, a misaligned device pointer, conflicting repeats, a null result of value_rows
 *   -> IVFHNSW_ERR_INVALID; set before upload_ivf, set or clear on a view, set / clear / a _values call on a handle with
 *   shard_world > 1 -> IVFHNSW_ERR_STATE; a failed allocation -> IVFHNSW_ERR_NOMEM; whatever search_dev /
 *   range_search_dev refuses for the same params -> that status.  An error leaves earlier range results and the
 *   installed state as they were.
 * An interval AND a tag per query: the _tags_values calls ("Row tags AND row values" below).
 * Not built: values for search_reconstruct, search_sharded and sharded handles; an interval AND a slot or the handle's
 *   filter; 64-bit or float values, or several values per row. */
#define IVFHNSW_VALUE_NONE 0xffffffffu
int ivfhnsw_gpu_set_values(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, const uint32_t *values);
int ivfhnsw_gpu_set_values_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, const uint32_t *d_values);
int ivfhnsw_gpu_clear_values(ivfhnsw_gpu *h);
int ivfhnsw_gpu_values_info(ivfhnsw_gpu *h, uint64_t *rows_valued, uint64_t *rows_total, uint64_t *table_labels);
int ivfhnsw_gpu_value_rows(ivfhnsw_gpu *h, uint32_t lo, uint32_t hi, uint64_t *rows);

/* Row tags AND row values: "the nearest neighbours among THIS tenant's vectors of the LAST HOUR" in one
 * call.  The _tags_values forms of search and range search take both per-query arrays of the two sections above:
 * query_tags [nq] uint16 and query_ranges [2 * nq] uint32, (lo, hi) of query q at [2q], [2q + 1].
 *   The rule: a row passes query q iff (t == IVFHNSW_TAG_NONE || tag(row) == t) && lo <= value(row) <= hi -- exactly the
 * AND of the two rules above, both wildcards kept: (NONE, (0, 0xffffffff)) is the unfiltered query, (t, (0, 0xffffffff))
 * the _tags query, (NONE, (lo, hi)) the _values query, and lo > hi passes nothing.
 *   Query q answers, bit for bit, what the plain call answers on the same handle with set_filter({labels tagged t whose
 * value lies in [lo, hi]}, ALLOW) installed, in everything the two sections above list; max_codes and Grouping's pruning
 * count every stored code and last_scan_counts is the unfiltered call's.  A launch reports the unfiltered kernel's name
 * with "+tags+values" appended and runs plan, table and scan as a _values launch does.  query_tags == NULL makes the call
 * the _values call ("+values"), query_ranges == NULL the _tags call, both NULL the plain call.
 *   No new state: the calls read the tags and the values the handle (a view: its parent) already holds and that every
 * update re-derives.  They ignore slots; with a set_filter filter installed -> IVFHNSW_ERR_STATE; on a handle that lacks
 * the tag table, the value table or both they are legal and the missing one reads as NONE for every row; on a handle with
 * shard_world > 1 -> IVFHNSW_ERR_STATE.  Host memory for the host forms; device memory for _dev, the tags 2-byte and the
 * ranges 8-byte aligned (else IVFHNSW_ERR_INVALID).  A host call stages 2 + 8 bytes per query.  Other errors are the
 * twins'; an error leaves earlier range results and all installed state as they were.
 *   ivfhnsw_gpu_tag_value_rows: *rows = resident rows the rule passes (size max_codes from it); tag > 0xffff or a null
 * result -> IVFHNSW_ERR_INVALID.
 * Not built: the exact calls under tag AND interval (the store would need a (tag, value, row) order); a slot or the
 *   handle's filter AND-ed with either; search_reconstruct, search_sharded and sharded handles; several tags or values
 *   per row. */
int ivfhnsw_gpu_tag_value_rows(ivfhnsw_gpu *h, unsigned tag, uint32_t lo, uint32_t hi, uint64_t *rows);

/* The extra members of IndexIVF_HNSW_Grouping (IndexIVF_HNSW_Grouping.h:17-22,61) after read()
 * (IndexIVF_HNSW_Grouping.cpp:445-483).  All [nc*nsubc] row major; subgroup_sizes rows of empty
 * groups are zero.  Requires upload_ivf first and upload_quantizer before searching. */
int ivfhnsw_gpu_upload_grouping(ivfhnsw_gpu *h, size_t nsubc, const float *alphas,
                                const uint32_t *nn_centroid_idxs, const uint32_t *subgroup_sizes,
                                const float *inter_centroid_dists);

/* The coarse quantizer: hnswlib::HierarchicalNSW node storage (hnswlib/hnswalg.h:47-82; link count,
 * maxM link slots and d floats per node, hnswalg.cpp:25-27) as three arrays.  `vectors` are the
 * centroids as the graph holds them at search time, i.e. after rotate_quantizer()
 * (IndexIVF_HNSW.cpp:789-800) when OPQ is on.  Needed for Grouping (sub-centroid distances,
 * IndexIVF_HNSW_Grouping.cpp:248,314) and for the on-device coarse walk. */
int ivfhnsw_gpu_upload_quantizer(ivfhnsw_gpu *h, size_t n, size_t d, size_t maxM, uint32_t enterpoint,
                                 const uint8_t *link_counts, const uint32_t *links, const float *vectors);

/* One query per call is how the reference's drivers search (tests/test_ivfhnsw_sift1b.cpp:193-208).  prepare_latency
 * builds, once per uploaded quantizer, the "fat" copy of the graph the latency form of the walk reads -- every node
 * with the float rows of its own neighbours, n * 32 * d * 4 bytes (16 GB at 993 127 centroids, d = 128): a whole
 * workgroup then walks one query with one memory round trip per expansion.  After it, calls with at most 256 queries
 * take that form (same results: tests/test_latency_gpu.py).  Needs d = 128 or 96, maxM <= 32, at most 2^20 nodes,
 * efSearch <= 256; otherwise IVFHNSW_ERR_INVALID and nothing changes.  upload_quantizer discards the copy. */
int ivfhnsw_gpu_prepare_latency(ivfhnsw_gpu *h);

/* Large batches as two uneven parts on two streams inside ivfhnsw_gpu_search[_dev] (a batched extension; the reference
 * searches one query per call, IndexIVF_HNSW.cpp:232-293).  permille = share of the batch in the first part, 1..999;
 * 1000, the default since ABI 9, = chosen per call from its own parameters (the walk's time against table + plan + scan:
 * 0.79 at (32, 10000, 80), 1.81 -> 1.67 ms per 10 k queries at the 1B shape; 0.63 at (64, 30000, 100); 0.49 for Grouping);
 * 0 = one part (the environment variable IVFHNSW_SPLIT sets the same at ivfhnsw_gpu_create).  The second part is a whole
 * number of 2048-query rounds, at most half the batch, and runs on an internal view of the handle;
 * its walk fills the tail of the first part's, the first part's table + scan run beside it.  Results, ordering behind
 * the handle's stream and error reporting are those of the unsplit call.  Applies to calls of >= 8192 queries without
 * given coarse results, out_keys or heap-order k > 1. */
int ivfhnsw_gpu_set_batch_split(ivfhnsw_gpu *h, int permille);
/* The queries in the two parts of the last search[_dev] call (second = 0: it ran in one part). */
int ivfhnsw_gpu_last_batch_parts(ivfhnsw_gpu *h, uint64_t *first, uint64_t *second);

/* Options of this library (nothing of the reference's: its knobs are public members, below).  Unknown keys are refused.
 *   "scan_pipe"  -1 (default) the library chooses, 0 never, 1 wherever the shape allows: table + scan of a list shard as
 *                ONE software-pipelined kernel (kernels_scan3.hip) instead of two kernels.  A caller that runs a sharded
 *                step as two overlapping parts (ShardedSearcher) turns it off: the pipelined form holds most of a CU's
 *                LDS and cannot run beside the other part's walk.
 *   "exact_splits"  -1 (default) the library chooses from (nq, n); 1..64: exact_search cuts the store's rows into that many
 *                column splits whose partial tables are merged.  The results are the same for every value; the key exists so
 *                that the split and merge path can be exercised on a small store.  Other values: IVFHNSW_ERR_INVALID.
 *                exact_range_search cuts the store the same way (its slices of a query follow each other in label order).
 *   "exact_range_map"  -1 (default) or 1: exact_range_search's first pass leaves a map of the tiles in which anything
 *                passed and its second pass visits only those; 0: the second pass sweeps the whole store again.  The
 *                results are the same; the key exists so that both can be measured and compared.
 *   "exact_filter_form"  -1 (default) the rule: under a base filter (below) the exact calls sweep the list of passing
 *                rows when at most n / 8 rows pass, else the store behind its pass bits; 0: always the pass bits; 1: always
 *                the list (built on demand whatever the number of passing rows).  The results are the same; the key exists
 *                so that both forms can be exercised on a small store and measured.  Other values: IVFHNSW_ERR_INVALID. */
int ivfhnsw_gpu_set_option(ivfhnsw_gpu *h, const char *key, long value);

/* The search-time knobs the drivers set as public members (IndexIVF_HNSW.h:61-62, hnswalg.h:69,
 * IndexIVF_HNSW_Grouping.h:18). */
typedef struct ivfhnsw_search_params {
    size_t nprobe;
    size_t max_codes;
    size_t efSearch;
    int do_pruning;
    int heap_order; /* k > 1 only: 0 = results ascending by (distance, scan position), k <= 1024; 1 = exactly the
                       array faiss's max-heap leaves behind (IndexIVF_HNSW.cpp:265,285-288), slot 0 = current worst,
                       for any k and any number of admitted codes (with out_keys: k <= 1024 and the 8192-entry
                       candidate stream of ivfhnsw_gpu_last_stream_dev) */
} ivfhnsw_search_params;

/* IndexIVF_HNSW::search / IndexIVF_HNSW_Grouping::search (IndexIVF_HNSW.cpp:234-296,
 * IndexIVF_HNSW_Grouping.cpp:188-363) for nq queries at once.  All pointers are HOST memory.
 *
 * coarse_ids / coarse_dists ([nq*nprobe], nearest first) are the result of the coarse stage when the
 * caller ran it, exactly IndexIVF_HNSW::search2 (IndexIVF_HNSW.cpp:453-492); coarse slots holding
 * 0xffffffff are skipped.  Pass NULL for both to run the HNSW walk (hnswalg.cpp:48-109,227-234) on
 * the device; that needs upload_quantizer and efSearch >= nprobe.
 *
 * Results: distances[nq*k], labels[nq*k] (int64, the reference's `long`); unfilled slots hold FLT_MAX / -1 as
 * after faiss::maxheap_heapify.  For k = 1 (every preset of the reference) this is exactly the reference's
 * output.  For k > 1 the same set is returned either ascending by (distance, scan position)
 * (params->heap_order = 0) or, with heap_order = 1, in exactly the heap-array order the reference leaves: the
 * device replays faiss's pop/push over a superset of the admitted codes in scan order, which yields the same
 * heap because a code that fails `dist < distances[0]` leaves the heap untouched.  k > 1024 is accepted in heap
 * order only; a query whose candidate stream outgrows 8192 entries is recomputed without one, so heap order has no
 * bound on k or on the admitted codes here (the heap moves to global memory when it does not fit in LDS beside the
 * query's table: exact, but slow). */
int ivfhnsw_gpu_search(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                       const float *coarse_dists, const ivfhnsw_search_params *params, float *distances,
                       int64_t *labels);

/* Same, with every buffer already resident in HBM (device pointers), asynchronous on the handle's
 * stream.  out_keys (nullable, [nq*k] int64) receives the packed (orderable distance << 32 | scan
 * position) keys, sign-flipped so that a plain signed int64 MIN over the shards (RCCL all-reduce) picks
 * the reference's winner: smallest distance, earliest scan position on ties. */
int ivfhnsw_gpu_search_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries,
                           const uint32_t *d_coarse_ids, const float *d_coarse_dists,
                           const ivfhnsw_search_params *params, float *d_distances, int64_t *d_labels,
                           int64_t *d_out_keys);

/* ivfhnsw_gpu_search / ivfhnsw_gpu_search_dev with a filter slot per query (see "Filter slots" above): query_slots [nq]
 * bytes, host memory for the host form, device memory for the _dev form; NULL = the plain call. */
int ivfhnsw_gpu_search_slots(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                             const float *coarse_dists, const ivfhnsw_search_params *params, const uint8_t *query_slots,
                             float *distances, int64_t *labels);
int ivfhnsw_gpu_search_slots_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                 const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                 const uint8_t *d_query_slots, float *d_distances, int64_t *d_labels, int64_t *d_out_keys);

/* ... and with a row tag per query (see "Row tags" above): query_tags [nq] uint16, host memory for the host form, device
 * memory (2-byte aligned) for the _dev form; NULL = the plain call. */
int ivfhnsw_gpu_search_tags(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                            const float *coarse_dists, const ivfhnsw_search_params *params, const uint16_t *query_tags,
                            float *distances, int64_t *labels);
int ivfhnsw_gpu_search_tags_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                const uint16_t *d_query_tags, float *d_distances, int64_t *d_labels, int64_t *d_out_keys);

/* ... and with a value interval per query (see "Row values" above): query_ranges [2 * nq] uint32, host memory for the
 * host form, device memory (8-byte aligned) for the _dev form; NULL = the plain call. */
int ivfhnsw_gpu_search_values(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                              const float *coarse_dists, const ivfhnsw_search_params *params, const uint32_t *query_ranges,
                              float *distances, int64_t *labels);
int ivfhnsw_gpu_search_values_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                  const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                  const uint32_t *d_query_ranges, float *d_distances, int64_t *d_labels, int64_t *d_out_keys);

/* ... and with both (see "Row tags AND row values" above); either array NULL = the other's call. */
int ivfhnsw_gpu_search_tags_values(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                                   const float *coarse_dists, const ivfhnsw_search_params *params, const uint16_t *query_tags,
                                   const uint32_t *query_ranges, float *distances, int64_t *labels);
int ivfhnsw_gpu_search_tags_values_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries, const uint32_t *d_coarse_ids,
                                       const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                       const uint16_t *d_query_tags, const uint32_t *d_query_ranges, float *d_distances,
                                       int64_t *d_labels, int64_t *d_out_keys);

/* Multi-GPU merge helper: given keys already MIN-reduced over the shards, resolve the
 * labels this shard owns ([nq*k]; -1 where the winner lives on another shard) from the scan plan of
 * the last search_dev call, and decode the distances.  The caller then MAX-reduces the labels. */
int ivfhnsw_gpu_resolve_keys_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const int64_t *d_keys,
                                 float *d_distances, int64_t *d_labels);

/* k > 1 across shards.  Ascending order: all-gather the out_keys of every shard and keep the k smallest
 * per query, then resolve.  The reference's heap-array order (IndexIVF_HNSW.cpp:265,285-288) needs the sequence of
 * admitted codes in scan order: search_dev with heap_order = 1 AND out_keys leaves each shard's candidate stream -- a
 * superset of the codes faiss's heap admits, in this shard's scan order, as (orderable distance << 32 | scan position)
 * keys -- copied out by last_stream_dev: d_len ([nq], nullable) receives the stream lengths, d_keys ([nq][len_cap],
 * nullable) the first len_cap keys of every query's stream, *stream_cap (nullable) the library's capacity; a length
 * above that capacity means the stream overflowed: use ascending order.  The caller merges the shards' streams by
 * scan position and hands the merged stream to replay_stream_dev, which replays faiss's pop/push over it and writes
 * the heap ARRAY as signed keys ([nq*k], unfilled slots = the FLT_MAX key); resolve_keys_dev + MAX-reduce then give
 * labels.  Replaying a superset in scan order is exact: a code failing `dist < distances[0]` leaves the heap as it is. */
int ivfhnsw_gpu_last_stream_dev(ivfhnsw_gpu *h, size_t nq, size_t len_cap, uint64_t *d_keys, uint32_t *d_len,
                                uint32_t *stream_cap);
int ivfhnsw_gpu_replay_stream_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const uint64_t *d_stream, const uint32_t *d_len,
                                  uint32_t cap, int64_t *d_out_keys);

/* Host-pointer forms of the shard step, for a caller that merges the shards itself in one process (the bundled classes
 * with IVFHNSW_SHARDS=N: N handles, one per GPU of the node).  search_keys = search_dev with out_keys on host buffers
 * (the coarse stage must be supplied: it is computed once for all shards); resolve_keys = resolve_keys_dev;
 * last_stream = last_stream_dev.  All synchronous. */
int ivfhnsw_gpu_search_keys(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                            const float *coarse_dists, const ivfhnsw_search_params *params, int64_t *keys);
int ivfhnsw_gpu_resolve_keys(ivfhnsw_gpu *h, size_t nq, size_t k, const int64_t *keys, float *distances,
                             int64_t *labels);
int ivfhnsw_gpu_last_stream(ivfhnsw_gpu *h, size_t nq, size_t len_cap, uint64_t *keys, uint32_t *lens,
                            uint32_t *stream_cap);

/* The whole shard step for a caller that holds the N shard handles of one index in ONE process (north_star: "per-shard
 * top-k merged over RCCL/xGMI" under C++ host code): every shard scans its lists for the batch (the coarse stage is
 * supplied: it is computed once, IndexIVF_HNSW::search2's split, IndexIVF_HNSW.cpp:453-492), the packed keys are
 * MIN-merged across the shards' devices with one RCCL all-reduce (ncclInt64 / ncclMin; RCCL is loaded on first use), each
 * shard resolves the labels it owns, one more all-reduce (ncclMax) merges them, and shard 0's device returns distances
 * and labels.  k = 1, or k > 1 ascending (heap_order = 0).  Shards that share a device (a one-GPU box) or k > 1: the same
 * step with the merge on the host.  Host pointers; at most 131 072 queries per call. */
int ivfhnsw_gpu_search_sharded(ivfhnsw_gpu *const *shards, size_t nshards, size_t nq, size_t k, const float *queries,
                               const uint32_t *coarse_ids, const float *coarse_dists, const ivfhnsw_search_params *params,
                               float *distances, int64_t *labels);

/* ---- range search ---------------------------------------------------------------------------------
 *
 * faiss's range_search (Index::range_search / RangeSearchResult: lims, distances, labels) for the lists the handle
 * holds: everything closer than the radius instead of the best k.  The candidates of a query are the codes the loop of
 * IndexIVF_HNSW.cpp:282-289 (Grouping: IndexIVF_HNSW_Grouping.cpp:321-333) meets, i.e. the codes ivfhnsw_gpu_search of the
 * same call would score: the same rotation, coarse stage (the walk, or coarse_ids / coarse_dists with 0xffffffff slots
 * skipped), probe order, max_codes rule, sub-groups and pruning decisions, and the label filter when one is installed
 * (a filtered row is never returned; max_codes and pruning count every stored code).  A candidate is returned iff
 * dist < radius -- strict, as faiss compares for L2; a NaN distance fails -- with dist bit for bit what
 * ivfhnsw_gpu_search returns for that code.  The results of one query stand in ascending scan position, the order in
 * which that loop meets them.  No cap per query, nothing truncated, nothing padded; radius = +inf returns every scored
 * code with a finite distance.
 *   lims [nq + 1]: lims[0] = 0, query q's results are entries [lims[q], lims[q + 1]) of distances (float) and labels
 *   (int64); *total = lims[nq].  The results stay in HBM the handle owns until its next range search, upload_ivf or
 *   destroy (a view holds its own); ivfhnsw_gpu_memory_bytes counts them (12 bytes per result, kept at their largest
 *   size so far, plus 4 bytes per (query, slice) of the count).
 *   params: nprobe, max_codes, efSearch and do_pruning as in ivfhnsw_gpu_search; heap_order is ignored.
 *   Both forms return when the results are complete, and synchronise the handle's stream ONCE between their two passes:
 *   the host has to size the result buffers from the count (as ivfhnsw_gpu_kmeans_dev reads its objective per
 *   iteration).  ivfhnsw_gpu_last_scan_counts reports what the k-search of the same arguments reports,
 *   ivfhnsw_gpu_last_scan_kernel the range kernel's name ("+filter" appended on a filtered launch).  A range search ends
 *   the validity of the last search's plan and candidate stream (resolve_keys*, last_stream*), as a removal does.
 *   Limits: a batch whose results number 2^32 or more -> IVFHNSW_ERR_INVALID with a message (nothing is returned: split
 *   the batch or lower the radius); at most 131 072 queries per call.
 *   Errors leave earlier range results as they were: NaN radius, NULL queries, NULL lims or total with nq > 0 ->
 *   IVFHNSW_ERR_INVALID; whatever ivfhnsw_gpu_search_dev refuses for the same params -> that call's status; before
 *   upload_ivf, or on a handle with shard_world > 1 (range search over the key protocol is not built) ->
 *   IVFHNSW_ERR_STATE; a failed allocation -> IVFHNSW_ERR_NOMEM.  nq = 0: lims[0] = 0, *total = 0, success.
 * ivfhnsw_gpu_range_search: host pointers.  ivfhnsw_gpu_range_search_dev: device pointers (d_lims 8-byte aligned), *total on
 *   the host.
 * ivfhnsw_gpu_range_results: copies entries [first, first + count) to host buffers (either may be NULL); first + count
 *   beyond the total -> IVFHNSW_ERR_INVALID; count = 0 succeeds.  ivfhnsw_gpu_range_results_dev: the device pointers
 *   themselves (NULL when the total is 0) and the total, each output nullable.  Either before any range search on the
 *   handle -> IVFHNSW_ERR_STATE. */
int ivfhnsw_gpu_range_search(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                             const float *coarse_dists, const ivfhnsw_search_params *params, float radius,
                             uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_range_search_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                 const float *d_coarse_dists, const ivfhnsw_search_params *params, float radius,
                                 uint64_t *d_lims, uint64_t *total);
/* ... and with a filter slot per query ("Filter slots" above); results are read with range_results as usual */
int ivfhnsw_gpu_range_search_slots(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                   const float *coarse_dists, const ivfhnsw_search_params *params, const uint8_t *query_slots,
                                   float radius, uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_range_search_slots_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                       const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                       const uint8_t *d_query_slots, float radius, uint64_t *d_lims, uint64_t *total);
/* ... and with a row tag per query ("Row tags" above) */
int ivfhnsw_gpu_range_search_tags(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                  const float *coarse_dists, const ivfhnsw_search_params *params, const uint16_t *query_tags,
                                  float radius, uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_range_search_tags_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                      const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                      const uint16_t *d_query_tags, float radius, uint64_t *d_lims, uint64_t *total);
/* ... and with a value interval per query ("Row values" above) */
int ivfhnsw_gpu_range_search_values(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                    const float *coarse_dists, const ivfhnsw_search_params *params, const uint32_t *query_ranges,
                                    float radius, uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_range_search_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                        const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                        const uint32_t *d_query_ranges, float radius, uint64_t *d_lims, uint64_t *total);
/* ... and with both ("Row tags AND row values" above) */
int ivfhnsw_gpu_range_search_tags_values(ivfhnsw_gpu *h, size_t nq, const float *queries, const uint32_t *coarse_ids,
                                         const float *coarse_dists, const ivfhnsw_search_params *params,
                                         const uint16_t *query_tags, const uint32_t *query_ranges, float radius, uint64_t *lims,
                                         uint64_t *total);
int ivfhnsw_gpu_range_search_tags_values_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, const uint32_t *d_coarse_ids,
                                             const float *d_coarse_dists, const ivfhnsw_search_params *params,
                                             const uint16_t *d_query_tags, const uint32_t *d_query_ranges, float radius,
                                             uint64_t *d_lims, uint64_t *total);
int ivfhnsw_gpu_range_results(ivfhnsw_gpu *h, uint64_t first, uint64_t count, float *distances, int64_t *labels);
int ivfhnsw_gpu_range_results_dev(ivfhnsw_gpu *h, const float **d_distances, const int64_t **d_labels, uint64_t *total);

/* ---- reconstruction of stored vectors ------------------------------------------------------------
 *
 * faiss's reconstruct / reconstruct_n / search_and_reconstruct and the label -> row lookup of its direct map, for the
 * lists the handle holds, without a download.  Read-only: tables, filter and range results stay as they are, and the
 * label filter plays no part (these calls address stored rows).
 *   Resident row r = position r of the handle's ids / codes / norm_codes arrays, in ivfhnsw_gpu_download_ivf order; list
 *   c is rows [offsets[c], offsets[c + 1]).  Rows stay valid until the next upload, append, add, remove or add_groups.
 *   Anchor of a row: with V the vectors given to ivfhnsw_gpu_upload_quantizer (with OPQ: the rotated centroids), V[c]
 *   for a row of list c; on a Grouping index, for a row of sub-group s of list c (s follows from the row's place in the
 *   list and subgroup_sizes[c]), cv = V[nn[c][s]] + (-1.f * V[c]), anchor = V[c] + alpha[c] * cv
 *   (IndexIVF_HNSW_Grouping.cpp:70-87).  Each step one float operation, nothing contracted.
 *   IVFHNSW_RECON_ROTATED: y[j] = anchor[j] + pq_centroids[m][code[m]][j - m * dsub], m = j / dsub; one add.
 *   IVFHNSW_RECON_ORIGINAL: without OPQ the same bits; with OPQ x[i] = sum over k of A[k][i] * y[k] as the k-ordered
 *   fmaf chain from 0.0f (transform_transpose), bit for bit what ivfhnsw_gpu_rotate_dev returns for y on a handle whose
 *   opq_A is the transpose of this one's.  NOT the reference's c + A^T * dec (IndexIVF_HNSW.cpp:106-113): a served handle
 *   holds only the rotated centroids, so the centroid goes through the float rotation and back; the two agree to the
 *   rounding of a d-term float sum (DESIGN.md 3.16 records the measured bound).
 *   Empty slot (row -1, a label that no row bears, an unfilled search result): d floats of bit pattern 0x7fc00000.
 * locate: rows[i] = the lowest resident row whose id equals labels[i], or -1; counts[i] (nullable) = the resident rows
 *   bearing that label.  Any label value (0xffffffff included); repeated labels in the request get the same answer each;
 *   n = 0 does nothing.  One pass over the ids against a bitmap of the labels (as ivfhnsw_gpu_remove_ids marks; at most
 *   512 MB), hits looked up in the sorted request.  The host form is synchronous; locate_dev (labels and counts 4-byte
 *   aligned, rows 8-byte) runs on the handle's stream and returns with it drained.  At most 2^31 - 1 labels per call.
 * reconstruct_rows: out [n][d] = the vectors of rows[0..n); row -1 is an empty slot.  Host form: a row outside
 *   [-1, n_local) -> IVFHNSW_ERR_INVALID and nothing written.  reconstruct_rows_dev (rows 8-byte aligned): such a row is
 *   an empty slot; asynchronous on the handle's stream.
 * reconstruct: locate followed by reconstruct_rows of the lowest row of every label; a label without a row gives an
 *   empty slot and counts in *n_missing (nullable).  reconstruct_dev returns with the stream drained when n_missing is
 *   given.
 * search_reconstruct: distances and labels bit for bit those of ivfhnsw_gpu_search / search_dev with the same arguments
 *   (filter, Grouping, pruning, heap_order as there); rows [nq*k] (nullable) = the resident row every result came from,
 *   -1 for an unfilled slot; recons [nq*k][d] = that row's reconstruction -- the winning row, not the first row bearing
 *   the label.  Runs search_dev with out_keys, so what that refuses is refused here with its status (heap_order with
 *   k > 1024), and with heap_order = 1 a query whose candidate stream outgrows 8192 entries is an IVFHNSW_ERR_STATE at
 *   the next synchronisation instead of being recomputed; large batches run in one part.  search_reconstruct_dev is
 *   asynchronous on the handle's stream.
 * Errors, all forms: before upload_ivf, the reconstructing forms before upload_quantizer or with a quantizer whose n or d
 *   differ from the index's nc or d, a handle with shard_world > 1 (a shard holds only its own lists) ->
 *   IVFHNSW_ERR_STATE; an unknown space, NULL buffers with n > 0, a misaligned device pointer -> IVFHNSW_ERR_INVALID; a
 *   failed allocation -> IVFHNSW_ERR_NOMEM.  Views are allowed: they read the parent's tables, the workspace is the
 *   view's.
 * Memory (kept on the handle, counted by ivfhnsw_gpu_memory_bytes): locate 20 bytes per label, the bitmap, 1 KB per 4096
 *   labels and, host form, 4 + 8 + 4 bytes per label of staging; reconstruction with OPQ in ORIGINAL space 4 d bytes per
 *   row of a chunk of 2^18 rows, host forms as much again for the output and 8 bytes per row; search_reconstruct 8 or 16
 *   bytes per result besides the search's own workspace. */
#define IVFHNSW_RECON_ORIGINAL 0
#define IVFHNSW_RECON_ROTATED 1
int ivfhnsw_gpu_locate(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int64_t *rows, uint32_t *counts);
int ivfhnsw_gpu_locate_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int64_t *d_rows, uint32_t *d_counts);
int ivfhnsw_gpu_reconstruct_rows(ivfhnsw_gpu *h, size_t n, const int64_t *rows, int space, float *out);
int ivfhnsw_gpu_reconstruct_rows_dev(ivfhnsw_gpu *h, size_t n, const int64_t *d_rows, int space, float *d_out);
int ivfhnsw_gpu_reconstruct(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int space, float *out, uint64_t *n_missing);
int ivfhnsw_gpu_reconstruct_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int space, float *d_out,
                                uint64_t *n_missing);
int ivfhnsw_gpu_search_reconstruct(ivfhnsw_gpu *h, size_t nq, size_t k, const float *queries, const uint32_t *coarse_ids,
                                   const float *coarse_dists, const ivfhnsw_search_params *params, int space,
                                   float *distances, int64_t *labels, int64_t *rows, float *recons);
int ivfhnsw_gpu_search_reconstruct_dev(ivfhnsw_gpu *h, size_t nq, size_t k, const float *d_queries,
                                       const uint32_t *d_coarse_ids, const float *d_coarse_dists,
                                       const ivfhnsw_search_params *params, int space, float *d_distances,
                                       int64_t *d_labels, int64_t *d_rows, float *d_recons);

/* The coarse stage alone (HierarchicalNSW::searchKnn, hnswalg.cpp:227-234, plus the unload loop of
 * IndexIVF_HNSW.cpp:249-259): device pointers, [nq*nprobe] outputs, nearest first.  Queries must
 * already be rotated when OPQ is on. */
int ivfhnsw_gpu_coarse_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, size_t nprobe, size_t efSearch,
                           uint32_t *d_coarse_ids, float *d_coarse_dists);

/* opq_matrix->apply (IndexIVF_HNSW.cpp:240) alone, device pointers: d_out[q] = A * d_queries[q].  A plain copy
 * when the index holds no OPQ matrix.  For callers that run the coarse stage themselves (sharded search). */
int ivfhnsw_gpu_rotate_dev(ivfhnsw_gpu *h, size_t nq, const float *d_queries, float *d_out);

/* Host-pointer form of the coarse stage; with k = 1 this is IndexIVF_HNSW::assign
 * (IndexIVF_HNSW.cpp:68-72) for n vectors.  The OPQ rotation is NOT applied (assign() takes vectors in
 * the graph's space).  Slots beyond the number of nodes found hold 0xffffffff / 0. */
int ivfhnsw_gpu_coarse(ivfhnsw_gpu *h, size_t nq, const float *queries, size_t k, size_t efSearch,
                       uint32_t *ids, float *dists);

/* ---- exact re-rank against the raw base vectors (IndexIVF_HNSW_Grouping::searchDisk) ------------------------------
 *
 * The raw base vectors the reference's searchDisk reads (utils.cpp:98-105: .bvecs records, uint32 dim + d bytes).
 * first == 0 (re)allocates n*d bytes, zero-filled, and frees any previous store; every call copies rows
 * [first, first+count): row r is read at rows + r*row_stride (row_stride >= d; d + 4 takes a .bvecs file image as it
 * is, `rows` pointing past the first record's 4-byte header).  n == 0 frees the store.  Needs d % 16 == 0,
 * 16 <= d <= 512 (fvec_L2sqr ignores a tail beyond 16*(d/16), utils.cpp:22-52) and n < 2^32; a later call whose n or d
 * differs from the store's: IVFHNSW_ERR_INVALID.  A failed allocation: IVFHNSW_ERR_NOMEM and no store.  Views see the
 * parent's store; ivfhnsw_gpu_memory_bytes counts it.  Synchronous: `rows` may be reused when the call returns.
 * upload_base_dev: the same with the rows already in HBM (device pointer). */
int ivfhnsw_gpu_upload_base(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const uint8_t *rows,
                            size_t row_stride);
int ivfhnsw_gpu_upload_base_dev(ivfhnsw_gpu *h, size_t n, size_t d, size_t first, size_t count, const uint8_t *d_rows,
                                size_t row_stride);

/* searchDisk's exact re-rank for nq queries (IndexIVF_HNSW_Grouping.cpp:365-395): d_cand[nq*kc] are labels a search
 * returned (-1 = empty), queries are unrotated (getL2Distance compares the raw query with the raw base row,
 * utils.cpp:98-137); writes the k best by (exact distance, label) ascending, [nq*k], padded with FLT_MAX / -1 when fewer
 * than k candidates are valid (IndexIVF_HNSW_Grouping.cpp:384-394).  Distance = fvec_L2sqr (utils.cpp:22-52) bit for
 * bit; duplicate labels stay duplicates; a label >= n counts as empty.  The reference sorts by `cmp` (utils.cpp:193-201),
 * which treats distances within 0.001 as equal: the same order whenever no two different distances of a query lie that
 * close, always so for integer-valued queries.  1 <= k <= kc <= 4096, else IVFHNSW_ERR_INVALID; no
 * store: IVFHNSW_ERR_STATE.  Device pointers, asynchronous on the handle's stream (ordered after a search_dev on the same
 * stream). */
int ivfhnsw_gpu_rerank_dev(ivfhnsw_gpu *h, size_t nq, size_t kc, const float *d_queries, const int64_t *d_cand,
                           size_t k, float *d_distances, int64_t *d_labels);
/* host pointers, synchronous; a candidate label outside [-1, n) -> IVFHNSW_ERR_INVALID, nothing written */
int ivfhnsw_gpu_rerank(ivfhnsw_gpu *h, size_t nq, size_t kc, const float *queries, const int64_t *cand,
                       size_t k, float *distances, int64_t *labels);

/* ---- exact brute-force search of the base store (the drivers' ground truth, -path_gt) ---------------------------------
 *
 * For each of nq queries the k rows of the base store (upload_base) nearest by exact squared L2, sum (q[j] - x[j])^2 in
 * integers, ascending by (distance, label), [nq*k], padded with FLT_MAX / -1 when the store has fewer than k rows.
 * Queries are uint8, d bytes each (the store's d), row_stride bytes apart (row_stride >= d; d + 4 takes a .bvecs query
 * file image as it is, `queries` pointing past the first record's header).  For d <= 256 the distance is at most
 * 256 * 255^2 < 2^24, so every partial sum of fvec_L2sqr (utils.cpp:22-52) is an exactly representable integer and the
 * float written is bit for bit what ivfhnsw_gpu_rerank returns for the same queries as floats with every row a
 * candidate; a store with d > 256: IVFHNSW_ERR_INVALID.  1 <= k <= 100, null buffers with nq > 0, row_stride < d:
 * IVFHNSW_ERR_INVALID; no store: IVFHNSW_ERR_STATE; nq = 0 does nothing; nq is unbounded (processed in chunks).  A view
 * searches its parent's store.  Neither form touches the index, the plan of the last search or its candidate stream; the
 * workspace belongs to the handle and ivfhnsw_gpu_memory_bytes counts it.
 * exact_search: host pointers, synchronous.  exact_search_dev: device pointers of any alignment, asynchronous on the
 * handle's stream (ordered after an upload_base_dev or search_dev on the same stream). */
int ivfhnsw_gpu_exact_search(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                             float *distances, int64_t *labels);
int ivfhnsw_gpu_exact_search_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                 float *d_distances, int64_t *d_labels);

/* ---- exact range search of the base store ----------------------------------------------------------
 *
 * Every row of the base store (upload_base) within a radius of each of nq queries: the true answer to the question
 * ivfhnsw_gpu_range_search answers approximately, in its layout (lims, distances, labels).  Queries as for exact_search:
 * uint8, the store's d bytes each, row_stride >= d bytes apart (d + 4 takes a .bvecs image as it is).
 *   Row j is returned for query q iff (float)dist(q, j) < radius, dist the integer sum (q[i] - x[i])^2 -- strict, as
 *   range_search and faiss compare for L2.  The distance written is that integer as a float, bit for bit what exact_search
 *   and rerank write for the pair (d <= 256: below 2^24, exact).  Every row of the store is a candidate, the zero rows of
 *   a chunk that was never uploaded included; the index's label filter (set_filter) does not apply, the base filter
 *   (set_base_filter, below) does.  The radius becomes an int32 threshold on the host, dist < thr: thr = 0 when
 *   !(radius > 0) (0, negatives, -inf: all-zero lims without a sweep), INT_MAX when radius > 2^24 (+inf), else
 *   (int)ceilf(radius) -- for integer dist < 2^24 exactly the float comparison.
 *   The results of one query stand in ASCENDING LABEL.  lims [nq + 1]: lims[0] = 0, query q owns entries
 *   [lims[q], lims[q + 1]) of distances (float) and labels (int64); *total = lims[nq].  No cap, nothing truncated or padded.
 *   The results stay in HBM the handle owns, apart from the IVF range search's (neither call disturbs the other's), until
 *   the handle's next exact range search or destroy: upload_base, exact_search and every index call leave them alone.  A
 *   view searches its parent's store and holds its own results.  The buffers keep their largest size so far.
 *   Memory (ivfhnsw_gpu_memory_bytes counts all of it): 12 bytes per result; 4 bytes per (query, column split) of the
 *   count; nq * d bytes of queries; and the tile map the first pass leaves for the second, one bit per (32 queries, 32
 *   rows) = nq * n / 8192 bytes, coarsened by powers of two until it is at most 1/16 of the store's n * d bytes (on a tiny
 *   store: 4 bytes per (32 queries, column split)).
 *   Both forms return when the results are complete, and synchronise the handle's stream ONCE between their two passes
 *   (the host sizes the results from the count, as range_search does).  With ivfhnsw_gpu_set_profiling the count pass is
 *   accounted as the scan stage and the fill pass as the select stage, as range_search accounts its own.
 *   Limits: at most 131 072 queries per call; 2^32 or more results in one call -> IVFHNSW_ERR_INVALID with a message,
 *   found after the count pass and before anything is allocated.
 *   Errors leave earlier results as they were: no store -> IVFHNSW_ERR_STATE; a store with d > 256, a NaN radius, NULL
 *   queries, lims or total with nq > 0, row_stride < d, more than 131 072 queries -> IVFHNSW_ERR_INVALID; a failed
 *   allocation -> IVFHNSW_ERR_NOMEM.  nq = 0: lims[0] = 0 (when lims is given), *total = 0, success.
 *   The options "exact_splits" and "exact_range_map" (ivfhnsw_gpu_set_option) apply; the results do not depend on them.
 * exact_range_search: host pointers.  exact_range_search_dev: device pointers (queries of any alignment, d_lims 8-byte
 *   aligned), *total on the host; ordered behind an upload_base_dev on the handle's stream.
 * exact_range_results[_dev]: as range_results[_dev], for these buffers: entries [first, first + count) to host buffers
 *   (either may be NULL; first + count beyond the total -> IVFHNSW_ERR_INVALID; count = 0 succeeds), or the device
 *   pointers themselves (NULL when the total is 0) and the total, each output nullable.  Either before any exact range
 *   search on the handle -> IVFHNSW_ERR_STATE. */
int ivfhnsw_gpu_exact_range_search(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, float radius,
                                   uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_exact_range_search_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, float radius,
                                       uint64_t *d_lims, uint64_t *total);
int ivfhnsw_gpu_exact_range_results(ivfhnsw_gpu *h, uint64_t first, uint64_t count, float *distances, int64_t *labels);
int ivfhnsw_gpu_exact_range_results_dev(ivfhnsw_gpu *h, const float **d_distances, const int64_t **d_labels, uint64_t *total);

/* ---- base filter: the exact calls under an allow or deny set of row numbers ---------------------------
 *
 * faiss's IDSelector for the flat search: the ground truth of a filtered search.  The handle that holds the store
 * (upload_base) holds no base filter or one: a set of uint32 labels and a mode (IVFHNSW_FILTER_ALLOW / IVFHNSW_FILTER_DENY).
 * A label is a ROW NUMBER of the store, the label exact_search returns.  Allow: a row passes iff its number is in the set;
 * deny: iff it is not.  Any uint32 value is accepted; labels >= n match nothing; repeats count once; an empty allow set
 * passes nothing, an empty deny set everything.
 * While a base filter is installed ivfhnsw_gpu_exact_search[_dev] and ivfhnsw_gpu_exact_range_search[_dev] answer as the
 * unfiltered call would on a store that held only the passing rows, the labels being the ORIGINAL row numbers: the same
 * distance bits, exact_search ascending by (distance, label) and padded with FLT_MAX / -1 when fewer than k rows pass, the
 * range search in ascending label per query with exact lims.  When no row passes neither call sweeps anything (padding;
 * all-zero lims and a total of 0).  Limits and errors of the unfiltered calls hold unchanged.  ivfhnsw_gpu_rerank* is not
 * touched: its candidates come from a search that was filtered already.  The index filter (ivfhnsw_gpu_set_filter, labels =
 * ids) and the base filter are independent: neither call sets, clears or reads the other, and the index filter never
 * applies to the exact calls.  Without a base filter nothing changes: the same kernels, the same bits.
 * The work follows the rows that pass.  The filter is kept as one pass bit per row (n / 8 bytes) and, when at most n / 8
 * rows pass, as the ascending list of the passing row numbers as well (4 bytes each, at most n / 2 bytes); the sweeps then
 * run over the list alone (cost in proportion to the passing rows), otherwise over the store, skipping every tile of 32
 * rows in which no row passes.  The option "exact_filter_form" (ivfhnsw_gpu_set_option) forces either form; results
 * never depend on it.  ivfhnsw_gpu_memory_bytes counts what the filter holds.
 *
 * ivfhnsw_gpu_set_base_filter replaces an earlier base filter; the new one is built on the device beside it and swapped
 *   in when complete, so any error leaves the earlier filter in force.  Synchronous on the handle's stream; needs a store
 *   (before upload_base: IVFHNSW_ERR_STATE) but no index; sharded handles are fine (the store is not sharded).  While
 *   it is built ~1 bit per label value up to the largest label (<= 512 MB) is allocated beside it.  n > 0 with NULL
 *   labels or an unknown mode: IVFHNSW_ERR_INVALID; a failed allocation: IVFHNSW_ERR_NOMEM.
 *   ivfhnsw_gpu_set_base_filter_dev: d_labels in device memory (4-byte aligned, else IVFHNSW_ERR_INVALID), read on the
 *   handle's stream.
 * ivfhnsw_gpu_clear_base_filter: no base filter afterwards; succeeds on a handle that has none.
 * ivfhnsw_gpu_upload_base[_dev] with first == 0 (a new store) or n == 0 (no store) drops the base filter; a later chunk
 *   (first > 0) keeps it.
 * Views: set / clear on a view -> IVFHNSW_ERR_STATE.  A view reads its parent's store at the call, and its parent's base
 *   filter the same way; replacing the filter (or uploading) while a view's exact call is in flight is the caller's to avoid.
 * ivfhnsw_gpu_base_filter_info: *mode = the installed mode or -1; *rows_passing = rows of the store that pass (all of them
 *   without a filter); *rows_total = rows of the store.  Each pointer nullable; a view reports its parent's. */
int ivfhnsw_gpu_set_base_filter(ivfhnsw_gpu *h, size_t n, const uint32_t *labels, int mode);
int ivfhnsw_gpu_set_base_filter_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_labels, int mode);
int ivfhnsw_gpu_clear_base_filter(ivfhnsw_gpu *h);
int ivfhnsw_gpu_base_filter_info(ivfhnsw_gpu *h, int *mode, uint64_t *rows_passing, uint64_t *rows_total);

/* ---- base filter slots: a base filter PER QUERY of an exact call --------------------------------------
 *
 * The truth of a _slots search ("Filter slots" above).  Beside its one base filter the handle that holds the store holds up
 * to IVFHNSW_FILTER_SLOTS (32) slots, each a set of uint32 ROW NUMBERS and a mode exactly as ivfhnsw_gpu_set_base_filter
 * takes them (any value, labels >= n match nothing, repeats count once, an empty allow set passes nothing, an empty deny
 * set everything).  A slot that was never set, or was cleared, passes nothing.  The _slots forms of both exact calls take
 * one byte per query: query q with query_slots[q] == s gets, bit for bit, what the plain call returns on the same handle
 * with set_base_filter(set of s, mode of s) installed -- exact_search: the original row numbers with the same distance
 * bits, ascending by (distance, label), padded with FLT_MAX / -1 when fewer than k rows pass; the range search: results per
 * query in ascending label, exact lims IN THE CALLER'S QUERY ORDER, held in the handle's exact-range buffers and read with
 * ivfhnsw_gpu_exact_range_results[_dev].  With IVFHNSW_SLOT_NONE (0xff) the query gets what the plain call returns with
 * no base filter.  query_slots == NULL is the plain call: same path, same kernels.
 *   Slots and the handle's base filter are independent state: plain calls never read slots, and a _slots call on a store
 * with a set_base_filter filter installed -> IVFHNSW_ERR_STATE (the two are not combined).
 *   The work follows each query's own passing rows: the queries of a call are grouped by slot into strips of 32 on the
 * device, every strip sweeps its own slot's rows in the form that slot is kept in (below), and one call takes at most
 * three sweep launches per chunk whatever the bytes are.  A group's last strip is padded to 32 rows.
 * ivfhnsw_gpu_set_base_filter_slot replaces the slot's earlier set; the new one is built beside the installed state and
 *   swapped in, so any error leaves every slot as it was.  Synchronous on the handle's stream.  _dev: d_labels in device
 *   memory (4-byte aligned).  ivfhnsw_gpu_clear_base_filter_slot: slot -1 = every slot; succeeds on a slot that is not set.
 *   ivfhnsw_gpu_upload_base[_dev] with first == 0 or n == 0 drops every slot; a later chunk (first > 0) keeps them.
 *   ivfhnsw_gpu_base_filter_slot_info: *mode = the slot's mode or -1, *rows_passing = rows of the store that pass it (0
 *   for a slot that is not set), *rows_total = rows of the store; each nullable; a view reports its parent's.
 * Query slot bytes: the host forms check them before anything is launched or written, a byte in 32..254 ->
 *   IVFHNSW_ERR_INVALID.  The _dev forms read nothing back: any byte other than 0xff that names no installed slot passes
 *   nothing.
 * Views: set / clear on a view -> IVFHNSW_ERR_STATE.  A view reads its parent's slots at the call.
 * Memory, all counted by ivfhnsw_gpu_memory_bytes: per installed slot its pass words, 4 * ceil(n / 32) bytes, and, when at
 *   most n / 8 of its rows pass, the ascending list of the passing rows as well (4 bytes each); once per store a table of 33
 *   entries of 16 bytes (allocated by the first set or the first _slots call) and the 8 bytes of the count's word the base
 *   filter shares; per calling handle the strip plans of its last _slots call (about 132 bytes per 32 queries) and a host
 *   form's staged bytes.  The option "exact_filter_form" applies per slot: 0 sweeps every slot behind its pass words, 1
 *   keeps and sweeps the list of every slot set while it is in force; the form a slot is swept in is the HOLDER's choice
 *   (a view's own option does not change it).  Results never depend on it.
 * Errors: slot >= IVFHNSW_FILTER_SLOTS, an unknown mode, NULL labels with n > 0, a misaligned d_labels ->
 *   IVFHNSW_ERR_INVALID; set or a _slots call before upload_base -> IVFHNSW_ERR_STATE; a failed allocation ->
 *   IVFHNSW_ERR_NOMEM; limits and errors of the plain calls hold unchanged, and whatever they refuse is refused with
 *   their status.
 * Not built: a slot AND the handle's base filter; more than 32 slots (disjoint sets beyond 32: "Base tags" below);
 *   filtering the re-rank's candidates; one bitmap shared between the index's filter slots and these. */
int ivfhnsw_gpu_set_base_filter_slot(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *labels, int mode);
int ivfhnsw_gpu_set_base_filter_slot_dev(ivfhnsw_gpu *h, unsigned slot, size_t n, const uint32_t *d_labels, int mode);
int ivfhnsw_gpu_clear_base_filter_slot(ivfhnsw_gpu *h, int slot); /* -1: every slot */
int ivfhnsw_gpu_base_filter_slot_info(ivfhnsw_gpu *h, unsigned slot, int *mode, uint64_t *rows_passing, uint64_t *rows_total);
int ivfhnsw_gpu_exact_search_slots(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                                   const uint8_t *query_slots, float *distances, int64_t *labels);
int ivfhnsw_gpu_exact_search_slots_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                       const uint8_t *d_query_slots, float *d_distances, int64_t *d_labels);
int ivfhnsw_gpu_exact_range_search_slots(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride,
                                         const uint8_t *query_slots, float radius, uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_exact_range_search_slots_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride,
                                             const uint8_t *d_query_slots, float radius, uint64_t *d_lims, uint64_t *total);

/* ---- base tags: a 16-bit tag per ROW OF THE STORE, a tag per query of an exact call --------------------
 *
 * The truth of a _tags search ("Row tags" above) in one call.  The handle that holds the store holds at most one base tag
 * array, one uint16 per store row; a row never tagged reads as IVFHNSW_TAG_NONE (0xffff).  The _tags forms of both exact
 * calls take one uint16 per query: query q with query_tags[q] == t, t != IVFHNSW_TAG_NONE, gets, bit for bit, what the
 * plain call returns on the same handle with set_base_filter({rows tagged t}, IVFHNSW_FILTER_ALLOW) installed --
 * exact_search: the original row numbers with the same distance bits, ascending by (distance, label), padded with FLT_MAX /
 * -1 when fewer than k rows carry t; the range search: results per query in ascending label, exact lims IN THE CALLER'S
 * QUERY ORDER, held in the handle's exact-range buffers and read with ivfhnsw_gpu_exact_range_results[_dev].  With
 * IVFHNSW_TAG_NONE the query gets what the plain call returns with no base filter.  A tag no row carries returns padding,
 * or an empty range.  query_tags == NULL is the plain call: same path, same kernels.  A _tags call on a store without a
 * tag array is legal: every row is IVFHNSW_TAG_NONE.
 *   Independent state: plain and _slots calls never read tags, a _tags call ignores base filter slots, and a _tags call on
 * a store with a set_base_filter filter installed -> IVFHNSW_ERR_STATE (the two are not combined).  The index's row tags
 * (ivfhnsw_gpu_set_tags) and the base tags never read each other.
 *   The work follows each query's own tag: the queries of a chunk are grouped by tag into strips of 32 on the device (a
 * stable sort of the chunk's query numbers by tag), the strips of the untagged queries sweep the whole store, every other
 * strip sweeps the ascending list of its tag's rows, and one call takes at most two sweep launches per chunk however
 * many tags its queries name.  A group's last strip is padded to 32 rows, so a chunk of m queries can take up to
 * m / 32 + min(m, tags in use + 1) strips: with many tags the padded rows, not the queries, size the workspace, and the
 * k-search shortens its chunk so that the partial tables stay within 256 MB.  One split count per call, from what the host
 * knows (the store's rows and the queries); every tagged strip sweeps in the list form, however many rows its tag holds.
 * ivfhnsw_gpu_set_base_tags mirrors ivfhnsw_gpu_set_tags with a ROW NUMBER of the store where that call has a label:
 *   incremental -- it (over)writes the tags of the rows given and leaves every other row alone; a row number >= n matches
 *   nothing; a repeat with the same tag counts once, one row given two different tags in one call -> IVFHNSW_ERR_INVALID;
 *   the tag IVFHNSW_TAG_NONE untags a row.  The new state is built beside the installed one and swapped in, so any error
 *   leaves the state as it was.  Synchronous on the handle's stream.  _dev: d_rows 4-byte and d_tags 2-byte aligned device
 *   memory, else IVFHNSW_ERR_INVALID (d_query_tags of the _dev calls: 2-byte aligned).
 *   ivfhnsw_gpu_clear_base_tags succeeds when there are none.  ivfhnsw_gpu_upload_base[_dev] with first == 0 or n == 0
 *   drops the tags; a later chunk (first > 0) keeps them.
 *   ivfhnsw_gpu_base_tags_info: *rows_tagged = rows whose tag is not IVFHNSW_TAG_NONE, *rows_total = rows of the store,
 *   *tags_in_use = tags at least one row carries; each nullable.  ivfhnsw_gpu_base_tag_rows: *rows = rows of the store that
 *   carry `tag` (tag <= 0xffff; IVFHNSW_TAG_NONE counts the untagged).
 * Views: set / clear on a view -> IVFHNSW_ERR_STATE.  A view reads its parent's tags at the call, and both info calls
 *   report the parent's.
 * Memory, all counted by ivfhnsw_gpu_memory_bytes: 2 n bytes of tags, 4 bytes per tagged row (the row numbers ordered by
 *   tag, then row) and 4 * 65537 bytes (256 KB) of their starts per tag: up to 6 n bytes, 6 GB on a store of 10^9 rows.  A
 *   set call takes 12 n bytes more while it runs (the sort) and frees them.  Per calling handle the strip plans of its last
 *   _tags call (144 bytes per strip), about 0.8 MB of plan workspace and a host form's staged 2 bytes per query.
 * Errors: NULL rows or tags with n > 0, a misaligned device pointer, conflicting repeats, tag > 0xffff in base_tag_rows ->
 *   IVFHNSW_ERR_INVALID; set, base_tag_rows or a _tags call before upload_base -> IVFHNSW_ERR_STATE; a failed allocation ->
 *   IVFHNSW_ERR_NOMEM; limits and errors of the plain calls hold unchanged, and whatever they refuse is refused with
 *   their status.
 * Not built: a tag AND the base filter or a slot; several tags per row or tags wider than 16 bits; a pass-word (masked)
 *   sweep for tags that hold a large share of the store; a split count per form; tags on the re-rank's candidates; one
 *   tag array shared between the index and the store. */
int ivfhnsw_gpu_set_base_tags(ivfhnsw_gpu *h, size_t n, const uint32_t *rows, const uint16_t *tags);
int ivfhnsw_gpu_set_base_tags_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_rows, const uint16_t *d_tags);
int ivfhnsw_gpu_clear_base_tags(ivfhnsw_gpu *h);
int ivfhnsw_gpu_base_tags_info(ivfhnsw_gpu *h, uint64_t *rows_tagged, uint64_t *rows_total, uint64_t *tags_in_use);
int ivfhnsw_gpu_base_tag_rows(ivfhnsw_gpu *h, unsigned tag, uint64_t *rows);
int ivfhnsw_gpu_exact_search_tags(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                                  const uint16_t *query_tags, float *distances, int64_t *labels);
int ivfhnsw_gpu_exact_search_tags_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                      const uint16_t *d_query_tags, float *d_distances, int64_t *d_labels);
int ivfhnsw_gpu_exact_range_search_tags(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride,
                                        const uint16_t *query_tags, float radius, uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_exact_range_search_tags_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride,
                                            const uint16_t *d_query_tags, float radius, uint64_t *d_lims, uint64_t *total);

/* ---- base values: a uint32 per ROW OF THE STORE, an interval per query of an exact call -----------------
 *
 * The truth of a _values search ("Row values" above) in one call.  The handle that holds the store holds at most one base
 * value array, one uint32 per store row; a row never given a value reads as IVFHNSW_VALUE_NONE (0xffffffff).  The _values
 * forms of both exact calls take one pair per query, query_ranges[2 q] = lo and query_ranges[2 q + 1] = hi: store row r
 * passes query q iff lo <= value(r) <= hi, unsigned and inclusive at both ends -- the rule of "Row values", with no special
 * value.  Query q gets, bit for bit, what the plain call returns on the same handle with set_base_filter({rows whose value
 * lies in [lo, hi]}, IVFHNSW_FILTER_ALLOW) installed -- exact_search: the original row numbers with the same distance
 * bits, ascending by (distance, label), padded with FLT_MAX / -1 when fewer than k rows pass; the range search: results
 * per query in ascending label, exact lims IN THE CALLER'S QUERY ORDER, held in the handle's exact-range buffers and read
 * with ivfhnsw_gpu_exact_range_results[_dev].  (0, 0xffffffff) is the plain unfiltered call's answer; lo > hi, or an
 * interval no row falls in, returns padding or an empty range.  query_ranges == NULL is the plain call: same path, same
 * kernels.  A _values call on a store without a value array is legal: every row is IVFHNSW_VALUE_NONE.
 *   Independent state: plain, _slots and _tags calls never read values, a _values call ignores base filter slots and base
 * tags, and a _values call on a store with a set_base_filter filter installed -> IVFHNSW_ERR_STATE (the two are not
 * combined).  The index's row values (ivfhnsw_gpu_set_values) and the base values never read each other.
 *   The work follows each query's own interval.  The holder keeps ALL row numbers ordered by (value, row), so an interval
 * is one window of positions of that order, found on the device by two binary searches per query.  A query whose window
 * is the whole store sweeps it with the unfiltered kernel; a query whose window is empty is not swept; the others are
 * sorted by their windows' starts and cut into strips of 32, and a strip sweeps the rows from its first window's start to
 * its furthest end while every one of its queries counts only the rows of ITS OWN window: at most two sweep launches and
 * m / 32 + 2 strips per chunk of m queries, however many distinct intervals they name.  Intervals far apart in one strip
 * sweep the rows between them without scoring them.  One split count per call, as for the _slots and _tags forms.  The
 * range form ends with a reorder of the held results to (query, label) when a windowed strip ran: 28 bytes and a little
 * more per result while it runs, freed before the call returns.
 * ivfhnsw_gpu_set_base_values mirrors ivfhnsw_gpu_set_base_tags with a value in place of a tag: incremental; a row number
 *   >= n matches nothing; a repeat with the same value counts once, one row given two different values in one call ->
 *   IVFHNSW_ERR_INVALID, found on the device before anything is swapped; the value IVFHNSW_VALUE_NONE un-values a row.  The
 *   new state is built beside the installed one and swapped in, so any error leaves the state as it was.  Synchronous on
 *   the handle's stream.  _dev: d_rows and d_values 4-byte aligned device memory, else IVFHNSW_ERR_INVALID; d_query_ranges
 *   of the _dev calls: 8-byte aligned, as in "Row values".
 *   ivfhnsw_gpu_clear_base_values succeeds when there are none.  ivfhnsw_gpu_upload_base[_dev] with first == 0 or n == 0
 *   drops the values; a later chunk (first > 0) keeps them.
 *   ivfhnsw_gpu_base_values_info: *rows_valued = rows whose value is not IVFHNSW_VALUE_NONE, *rows_total = rows of the
 *   store; each nullable.  ivfhnsw_gpu_base_value_rows: *rows = rows of the store whose value lies in [lo, hi] (valueless
 *   rows count at 0xffffffff), the size of the window the calls sweep.
 * Views: set / clear on a view -> IVFHNSW_ERR_STATE.  A view reads its parent's values at the call, and both info calls
 *   report the parent's.
 * Memory, all counted by ivfhnsw_gpu_memory_bytes: 4 n bytes of values and 4 n bytes of row numbers, 8 GB on a store of
 *   10^9 rows; no sorted copy of the values is kept (a window's search reads values through the row order).  A set call
 *   takes 12 n bytes more while it runs (the new values and the sort's two permutations, one of which stays) and frees
 *   what it replaces.  Per calling handle the strip plans of its last _values call (400 bytes per strip), about 0.4 MB of
 *   plan workspace and a host form's staged 8 bytes per query.
 * Errors: NULL rows or values with n > 0, a misaligned device pointer, conflicting repeats, a NULL result ->
 *   IVFHNSW_ERR_INVALID; set, base_value_rows or a _values call before upload_base -> IVFHNSW_ERR_STATE; a failed
 *   allocation -> IVFHNSW_ERR_NOMEM; limits and errors of the plain calls hold unchanged, and whatever they refuse is
 *   refused with their status.
 * Not built: an interval AND the base filter, a slot or a tag; cost-aware grouping of the queries into strips (a strip
 *   sweeps from its first window's start to its furthest end); a split count per form; 64-bit values; the class surface. */
int ivfhnsw_gpu_set_base_values(ivfhnsw_gpu *h, size_t n, const uint32_t *rows, const uint32_t *values);
int ivfhnsw_gpu_set_base_values_dev(ivfhnsw_gpu *h, size_t n, const uint32_t *d_rows, const uint32_t *d_values);
int ivfhnsw_gpu_clear_base_values(ivfhnsw_gpu *h);
int ivfhnsw_gpu_base_values_info(ivfhnsw_gpu *h, uint64_t *rows_valued, uint64_t *rows_total);
int ivfhnsw_gpu_base_value_rows(ivfhnsw_gpu *h, uint32_t lo, uint32_t hi, uint64_t *rows);
int ivfhnsw_gpu_exact_search_values(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride, size_t k,
                                    const uint32_t *query_ranges, float *distances, int64_t *labels);
int ivfhnsw_gpu_exact_search_values_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride, size_t k,
                                        const uint32_t *d_query_ranges, float *d_distances, int64_t *d_labels);
int ivfhnsw_gpu_exact_range_search_values(ivfhnsw_gpu *h, size_t nq, const uint8_t *queries, size_t row_stride,
                                          const uint32_t *query_ranges, float radius, uint64_t *lims, uint64_t *total);
int ivfhnsw_gpu_exact_range_search_values_dev(ivfhnsw_gpu *h, size_t nq, const uint8_t *d_queries, size_t row_stride,
                                              const uint32_t *d_query_ranges, float radius, uint64_t *d_lims, uint64_t *total);

/* ---- measurement ------------------------------------------------------------------------------ */

/* ---- construction side: what IndexIVF_HNSW::add_batch computes before it appends --------
 *
 * ivfhnsw_gpu_upload_codebooks: the residual code book (faiss::ProductQuantizer, [M][256][d/M] floats), the norm
 * code book (ProductQuantizer(1,1,8): 256 floats) and the OPQ matrix (row major [d][d], NULL = no OPQ).
 * Independent of upload_ivf: an index under construction has no lists yet.  upload_quantizer must have
 * been called as well (the centroid rows are the graph's vectors).
 *
 * ivfhnsw_gpu_encode replaces IndexIVF_HNSW.cpp:75-121 for n base vectors (host pointers):
 *   idx      = precomputed_idx, or assign(n, x) = searchKnn(x, 1) with efSearch (:68-72) when NULL
 *   residual = x - centroid[idx]                     (fvec_madd, :258-262)
 *   codes    = pq->compute_codes([A] residual)       (:92-93)
 *   norm     = || centroid[idx] + [A^T] pq->decode(codes) ||^2,  norm_codes = norm_pq->compute_codes(norm)
 * out_idx may be NULL; out_codes [n*code_size]; out_norm_codes [n].  The caller appends them to its lists
 * (:122-131).  Bytes out: compared bit for bit with the CPU restatement in tests/test_gpu_encode.py. */
int ivfhnsw_gpu_upload_codebooks(ivfhnsw_gpu *h, size_t d, size_t code_size, const float *pq_centroids,
                                 const float *norm_table, const float *opq_A);
int ivfhnsw_gpu_encode(ivfhnsw_gpu *h, size_t n, const float *x, const uint32_t *precomputed_idx, size_t efSearch,
                       uint32_t *out_idx, uint8_t *out_codes, uint8_t *out_norm_codes);

/* ivfhnsw_gpu_encode_groups replaces IndexIVF_HNSW_Grouping::add_group (IndexIVF_HNSW_Grouping.cpp:43-125, up to
 * the distribution loops) for ngroups groups at once; group g is centroid centroid_idx[g] with the points
 * x[offsets[g] .. offsets[g+1]) (host pointers, offsets[0] = 0).  Per group:
 *   nn_centroid_idxs = searchKnn(centroid, nsubc + 1) with efSearch, minus the nearest          (:47-62)
 *   alpha            = compute_alpha over the group's points                                    (:691-733)
 *   sub-centroid s   = centroid + alpha * (neighbour_s - centroid)                              (:70-87)
 *   subcentroid_idx  = first nearest sub-centroid of every point                                (:673-689)
 *   codes, norm_codes as in ivfhnsw_gpu_encode with the sub-centroid in place of the centroid   (:93-125)
 * out_nn_centroid_idxs [ngroups*nsubc]; out_alphas [ngroups] (written only for groups with points: an empty
 * group keeps the caller's value, :63-64); out_subcentroid_idxs [n]; out_codes [n*code_size]; out_norm_codes [n].
 * The caller lays each list out sub-group by sub-group in arrival order and records the sub-group sizes
 * (:127-155).  Needs efSearch >= nsubc + 1; a walk that finds fewer centroids is an error. */
int ivfhnsw_gpu_encode_groups(ivfhnsw_gpu *h, size_t ngroups, size_t nsubc, const uint32_t *centroid_idx,
                              const uint64_t *offsets, const float *x, size_t efSearch, uint32_t *out_nn_centroid_idxs,
                              float *out_alphas, uint32_t *out_subcentroid_idxs, uint8_t *out_codes,
                              uint8_t *out_norm_codes);

/* ---- code-book training -------------------------------------------------------------------
 *
 * ivfhnsw_gpu_pq_train: the Lloyd iterations behind faiss::ProductQuantizer::train, which IndexIVF_HNSW::train_pq
 * (IndexIVF_HNSW.cpp:536-593) and IndexIVF_HNSW_Grouping::train_pq (IndexIVF_HNSW_Grouping.cpp:486-560) call on
 * residuals: niter iterations on n points x [n][d] (host), centroids [M][256][d/M] in and out (host).  Assignment =
 * pq->compute_codes with the current code book (first nearest code word, faiss's SSE order), update = mean of the
 * assigned sub-vectors with the sum taken in point order in float, code words nothing was assigned to stay.
 * out_assign (nullable) [n][M]: the last iteration's assignments.  Needs no upload.  faiss's own clustering (its
 * sampling, its random stream, its empty-cluster splits) is not reproduced: spec-level, parity unpinned.
 *
 * ivfhnsw_gpu_xty: C[a][b] = sum_i X[i][a] * Y[i][b] ([n][d] each, host; C [d][d]): the product behind the orthogonal
 * Procrustes step of faiss::OPQMatrix::train, on the matrix cores (v_mfma_f32_32x32x2_f32).  Order: fmaf chains over
 * chunks of IVFHNSW_XTY_CHUNK points, the chunks' partial products added in chunk order. */
#define IVFHNSW_XTY_CHUNK 2048
int ivfhnsw_gpu_pq_train(ivfhnsw_gpu *h, size_t n, size_t d, size_t M, const float *x, size_t niter, float *centroids,
                         uint8_t *out_assign);
int ivfhnsw_gpu_xty(ivfhnsw_gpu *h, size_t n, size_t d, const float *X, const float *Y, float *C);

/* ivfhnsw_gpu_kmeans: exact Lloyd k-means of the IVF coarse centroids, the input the reference never learns (its
 * drivers read it as -path_centroids and hand it to IndexIVF_HNSW::build_quantizer, IndexIVF_HNSW.cpp:34-66; the
 * README points to downloaded files).  x [n][d] (host); centroids [nc][d] (host) are the seeds in and the result out;
 * out_assign (nullable) [n]: the last iteration's assignment; out_obj (nullable, host) [niter]: each iteration's
 * objective.  One iteration, exactly:
 *   1. assign[i], dist[i] = the k = 1 result of ivfhnsw_gpu_knn (IVFHNSW_KNN_ALL) of x against the current centroids:
 *      (norm(x) + norm(c)) - 2 * dot with fmaf-chain norms and dots, ties to the lower id;
 *   2. obj[t] = sum of dist[i] in double (order free);
 *   3. every cluster with cnt > 0: component j = S / (float)cnt rounded once, S the float sum of the members' component
 *      j in ascending point index from 0.0f (lloyd_update_kernel's rule); an empty cluster keeps its row;
 *   4. empty clusters ci, ascending (faiss's split_clusters, its random pick made deterministic): cj = the cluster with
 *      the largest current count, ties to the lower id (counts changed by earlier splits of this iteration count);
 *      row ci = row cj; then for even j c[ci][j] *= 1 + EPS and c[cj][j] *= 1 - EPS, for odd j the other way round
 *      (EPS = 1/1024, float); cnt[ci] = cnt[cj] / 2, cnt[cj] -= cnt[ci].  The pairs are applied in that order.
 * Limits: 1 <= nc <= n < 2^31, d a multiple of 4 with d <= 128 (knn's).  niter = 0 returns the seeds unchanged and
 * writes nothing else.  Anything else, or a NULL x / centroids, returns IVFHNSW_ERR_INVALID and touches no buffer.
 * A point with no finite distance (NaN / inf input) returns IVFHNSW_ERR_STATE.  Needs no upload, and leaves the index
 * the handle holds as it was.
 * ivfhnsw_gpu_kmeans_dev: the same on device pointers (16-byte aligned) on the handle's stream; out_obj stays host
 * memory.  Synchronises once per iteration (the counts come to the host, where the splits are chosen) and returns when
 * it is done. */
int ivfhnsw_gpu_kmeans(ivfhnsw_gpu *h, size_t n, size_t d, size_t nc, const float *x, size_t niter, float *centroids,
                       uint32_t *out_assign, double *out_obj);
int ivfhnsw_gpu_kmeans_dev(ivfhnsw_gpu *h, size_t n, size_t d, size_t nc, const float *d_x, size_t niter, float *d_centroids,
                           uint32_t *d_out_assign, double *out_obj);

/* ---- exact nearest-neighbour tables and graph construction -------------------------------------
 *
 * ivfhnsw_gpu_knn: for each of nq query rows the k nearest of nx base rows by brute force on the matrix cores -- the exact
 * form of what the reference's construction side approximates with graph searches (a new node's link candidates,
 * hnswlib/hnswalg.cpp:212-225 -> :48-109; the nsubc + 1 nearest centroids of a centroid,
 * IndexIVF_HNSW_Grouping.cpp:47-62) and of the ground-truth files its drivers score Recall@1 against
 * (tests/test_ivfhnsw_sift1b.cpp:173-215).  Host pointers; queries == NULL means the base rows themselves (nq = nx).
 * mode: IVFHNSW_KNN_ALL every base row is a candidate; IVFHNSW_KNN_NOT_SELF row i of the base is no candidate of query
 * i (a neighbour table); IVFHNSW_KNN_EARLIER only base rows j < i are candidates of query i (the table an incremental
 * construction sees: node i against the nodes inserted before it).  d a multiple of 4, at most 128; k <= 80.
 * Arithmetic: dist = (norm(q) + norm(x)) - 2 * dot(q, x) with norm and dot as fmaf chains over k = 0..d-1 (what
 * v_mfma_f32_32x32x2_f32 computes); results ascending by (dist, id), slots beyond the candidates that exist hold
 * 0xffffffff / FLT_MAX.  out_dists may be NULL.
 * ivfhnsw_gpu_knn_dev: the same on device pointers, asynchronous on the handle's stream (d_queries may equal d_base). */
#define IVFHNSW_KNN_ALL 0
#define IVFHNSW_KNN_NOT_SELF 1
#define IVFHNSW_KNN_EARLIER 2
int ivfhnsw_gpu_knn(ivfhnsw_gpu *h, size_t nq, size_t nx, size_t d, const float *queries, const float *base, size_t k,
                    int mode, uint32_t *out_ids, float *out_dists);
int ivfhnsw_gpu_knn_dev(ivfhnsw_gpu *h, size_t nq, size_t nx, size_t d, const float *d_queries, const float *d_base,
                        size_t k, int mode, uint32_t *d_out_ids, float *d_out_dists);

/* ivfhnsw_gpu_build_graph: hnswlib::HierarchicalNSW::addPoint for ALL n nodes at once (hnswlib/hnswalg.cpp:212-225 as
 * IndexIVF_HNSW::build_quantizer loops it, IndexIVF_HNSW.cpp:34-66), with ONE deviation: a node's link candidates are
 * its EXACT ncand nearest among the nodes inserted before it (ivfhnsw_gpu_knn, IVFHNSW_KNN_EARLIER, on the matrix cores)
 * instead of the efConstruction results of a greedy search of the graph built so far (hnswalg.cpp:221 -> :48-109).
 * Everything after the candidates is the reference's: getNeighborsByHeuristic down to M links (:110-146, distances by
 * fstdistfunc, :326-357), the links stored farthest first (:153-170), and mutuallyConnectNewElement's reverse links in
 * insertion order -- appended while the neighbour has room, else the neighbour's maxM + 1 candidates shrunk by the same
 * heuristic (:171-209).  Because the candidates no longer depend on the graph, node t's final list is a fold over the
 * later nodes that chose t, in their order: every node is processed independently, and the result is exactly what the
 * serial loop would leave.  All of it runs on the device (kernels_graph.hip): the forward heuristic and the fold take one
 * node per wavefront, the reverse lists are a stable sort of the forward links; the library starts no host thread.
 * vectors [n][d] host; out_counts [n] (the 1-byte link count of hnswalg.cpp:25); out_links [n][maxM], zero from each
 * node's count on.  1 <= M <= maxM <= 64, M <= ncand <= 80, d a multiple of 16 with d <= 128, n < 2^31 and n * M < 2^32;
 * anything else, or a NULL argument, returns IVFHNSW_ERR_INVALID and touches no buffer.  n <= 1 writes zeros.
 * ivfhnsw_gpu_build_graph_dev: the same on device pointers (d_vectors 16-byte aligned as for kmeans_dev, d_out_links
 * 4-byte aligned, else IVFHNSW_ERR_INVALID), the one deviation from hnswalg.cpp:110-225 being the same: exact candidates.
 * Asynchronous on the handle's stream, as knn_dev: it reads nothing back (the reverse lists are bounded by n * M entries)
 * and does not synchronise; d_vectors is only read.  Needs no upload, and leaves the index, the last search's plan and
 * the candidate stream as they were; its workspace (the n x ncand table, n x M forward links and three arrays of that
 * size for the sort) stays on the handle and counts in ivfhnsw_gpu_memory_bytes.  The host-pointer form is an upload,
 * this call and a download.
 * ivfhnsw_gpu_last_graph_longest_reverse: the longest reverse list (later nodes that chose one node) the handle's last
 * build_graph[_dev] met, 0 before any; synchronises the stream. */
int ivfhnsw_gpu_build_graph(ivfhnsw_gpu *h, size_t n, size_t d, const float *vectors, size_t M, size_t maxM, size_t ncand,
                            uint8_t *out_counts, uint32_t *out_links);
int ivfhnsw_gpu_build_graph_dev(ivfhnsw_gpu *h, size_t n, size_t d, const float *d_vectors, size_t M, size_t maxM,
                                size_t ncand, uint8_t *d_out_counts, uint32_t *d_out_links);
int ivfhnsw_gpu_last_graph_longest_reverse(ivfhnsw_gpu *h, uint64_t *out);

enum ivfhnsw_stage {
    IVFHNSW_STAGE_OPQ = 0,    /* opq_matrix->apply, IndexIVF_HNSW.cpp:240 */
    IVFHNSW_STAGE_COARSE = 1, /* quantizer->searchKnn, :248 */
    IVFHNSW_STAGE_LUT = 2,    /* pq->compute_inner_prod_table, :262 */
    IVFHNSW_STAGE_PLAN = 3,   /* probe order + max_codes rule, :267-292 / Grouping.cpp:222-262 */
    IVFHNSW_STAGE_SCAN = 4,   /* the ADC loop, :282-289 */
    IVFHNSW_STAGE_SELECT = 5, /* label resolution */
    IVFHNSW_STAGE_COUNT = 6
};
/* With profiling on, every search brackets each stage with hipEvents on the launch stream: enabled = 1 every stage,
 * 2 only the scan, the kernel the roofline is about (an event pair costs about 7 us of stream time; six of them are
 * 2 % of a 10 k-query step), 0 off. */
int ivfhnsw_gpu_set_profiling(ivfhnsw_gpu *h, int enabled);
/* Accumulated since the last reset: milliseconds and number of launches of one stage. */
int ivfhnsw_gpu_get_stage_ms(ivfhnsw_gpu *h, int stage, double *ms_total, uint64_t *launches);
int ivfhnsw_gpu_reset_stage_ms(ivfhnsw_gpu *h);
/* Accounting of the last search on this handle: codes scored by this shard (the reference's `ncode`,
 * IndexIVF_HNSW.cpp:290, summed over the batch) and (sub)lists scored.  Synchronises. */
int ivfhnsw_gpu_last_scan_counts(ivfhnsw_gpu *h, uint64_t *ncodes, uint64_t *nsegments);
/* Name of the scan kernel the last search on this handle launched (the dominant kernel of the path: bench.py
 * reports its roofline under this name).  Never NULL; empty before the first search. */
const char *ivfhnsw_gpu_last_scan_kernel(ivfhnsw_gpu *h);
/* Bytes of HBM currently held by the handle. */
int ivfhnsw_gpu_memory_bytes(ivfhnsw_gpu *h, uint64_t *bytes);

#ifdef __cplusplus
}
#endif
#endif
