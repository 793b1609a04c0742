/*
 * rass_engine.h — C ABI of the MI355X-native embedding + vector-search engine
 * that drops in behind RASSEngine's embed_*() functions and OpenSearchIndexer
 * k-NN lookup.
 *
 * The reference has no FFI for this path: its boundary is HTTP/JSON to Ollama
 * (app/main.py:225-237) and to the OpenSearch k-NN plugin (app/main.py:1552).
 * Every entry point below names the reference call site whose arithmetic it
 * replaces.  The Python shim (rassengine_amd/) binds these with ctypes and is
 * the only caller; see INTEGRATION.md for the reference-side rebinding.
 *
 * Conventions
 *   - plain pointers and sizes only; no torch / C++ types cross this boundary
 *   - every function returns RASS_OK (0) or a negative rass_status; the text of
 *     the last failure on the calling thread is rass_last_error()
 *   - nothing throws across the ABI
 *   - "d_" parameters are device (HBM) pointers, everything else is host memory
 *   - `stream` parameters are a hipStream_t passed as void* (NULL = the
 *     engine's own stream / the null stream for the stateless kernels)
 *   - one engine drives ONE GPU; multi-GPU is one process per GPU (RCCL via
 *     torch.distributed in the Python layer), never several devices per engine
 */
#ifndef RASS_ENGINE_H
#define RASS_ENGINE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RASS_ABI_VERSION 1

typedef enum rass_status {
    RASS_OK = 0,
    RASS_ERR_INVALID = -1,     /* bad argument (shape, k, dtype, NULL) */
    RASS_ERR_HIP = -2,         /* a HIP runtime call failed */
    RASS_ERR_OOM = -3,         /* device or host allocation failed */
    RASS_ERR_NOT_FOUND = -4,   /* unknown index name / row */
    RASS_ERR_UNSUPPORTED = -5, /* valid request this build cannot serve */
    RASS_ERR_IO = -6           /* save/load failure */
} rass_status;

/* Corpus storage dtype.  RASS_F32 is the parity path (exact fp32 MFMA, bit-equal to the
 * oracle's fmaf-order emulation).  RASS_BF16 is a first-class bf16-ONLY corpus: rows are normalised in fp32, rounded
 * to bf16 and stored in the "tile16b" layout (half the HBM per row, half the bytes per scan); a search rounds the
 * normalised queries to bf16 and runs v_mfma_f32_16x16x32_bf16 with fp32 accumulation, so a returned score is the
 * fp32-accumulated dot product of the two bf16-rounded unit vectors (|error| vs the fp32 cosine ~1e-3, the
 * north_star tolerance; recall@k vs the fp32 index is measured, bench.py --corpus-dtype bf16).  Needs dim padded to
 * a multiple of 256; masked filters and k > RASS_MAX_K work as on an fp32 index (the bf16 scan's EXT variant); the
 * prefilter mode and the IVF build are fp32-only. */
typedef enum rass_dtype {
    RASS_F32 = 0,
    RASS_BF16 = 1,
    RASS_I8 = 2     /* ONLY as the slab_dtype of rass_ivf_build_ex / _prefix (an index is fp32 or bf16) */
} rass_dtype;

/* Limits of the fused scan kernel. */
#define RASS_MAX_K 32        /* top-k kept in one half-wave sorted list */
#define RASS_MAX_QBATCH 32   /* queries per scan launch (two 16-wide MFMA N tiles) */
#define RASS_MAX_K_MULTIPASS 4096 /* rass_index_search_ex: k > RASS_MAX_K is served in passes of RASS_MAX_K */
#define RASS_MAX_DEVICE_BATCH 4096 /* queries per rass_index_search_device_batch call */
#define RASS_MAX_MMR_FETCH 128 /* rass_index_search_mmr: candidates per query; rass_index_rows_gram: rows per list */
/* Row tag layout used by the Python shim (the engine itself only compares integers): bits 0..23 the
 * patientId dictionary code (0 = none), bits 24..30 the doc_type code (0 = none).  A masked filter
 * (rass_index_search_ex) selects on either field or both with one compare. */
#define RASS_TAG_PATIENT_MASK 0x00ffffff
#define RASS_TAG_DOCTYPE_SHIFT 24
#define RASS_TAG_DOCTYPE_MASK 0x7f000000
#define RASS_ROW_TAG_DELETED (-1)
/* Attribute columns of a flat index (rass_index_set_attr) and the predicates over them (rass_index_allow_from_attr_clauses). */
#define RASS_MAX_ATTRS 8              /* int32 columns per index */
#define RASS_ATTR_MISSING INT32_MIN   /* "this row has no value": every other int32 is a value */
#define RASS_MAX_ATTR_CLAUSES 64      /* clauses per query per rass_index_allow_from_attr_clauses call */
#define RASS_ATTR_ALL 0               /* mode: a row is allowed when ALL of the query's clauses hold */
#define RASS_ATTR_ANY 1               /*       ... when at least one does */
#define RASS_ATTR_REPLACE 0           /* combine: the result overwrites the bitmap */
#define RASS_ATTR_AND 1               /*          ... is ANDed into what the bitmap holds */
#define RASS_ATTR_OR 2                /*          ... is ORed into it */
#define RASS_ATTR_ANDNOT 3            /* rass_index_allow_combine only: dst & ~src */
#define RASS_KEY_NONE (-1)            /* key column: this row is in no group (every negative key reads so) */
#define RASS_MAX_KEY_EDGES 4097       /* rass_index_keys_from_attr_edges: RASS_MAX_K_MULTIPASS buckets */
#define RASS_QFILTER_NONE (-1)

typedef struct rass_engine rass_engine_t;
typedef struct rass_index rass_index_t;

/* ------------------------------------------------------------------ misc */

int rass_abi_version(void);
/* Thread-local text of the last error on this thread ("" if none). */
const char* rass_last_error(void);
/* Number of visible HIP devices, or a negative rass_status. */
int rass_device_count(void);

/* ---------------------------------------------------------------- engine */

/* One engine per process per GPU.  `dim` = EMBED_DIM (app/main.py:80), 1 .. 2048.  Up to 1024 columns every feature of
 * this header applies; a WIDE-row engine (1024 < dim <= 2048: what an encoder of hidden size 1536 / 2048 emits) serves
 * fp32 flat indices — add / delete / get / save / load and every search entry point incl. masked filters and k > 32 —
 * (and, for k <= 16, by the int8 prefilter mode: rass_index_set_prefilter), while a bf16 corpus, the bf16 prefilter, the IVF
 * build and cross-index batches answer RASS_ERR_UNSUPPORTED. */
int rass_engine_create(int device, int dim, rass_engine_t** out);
void rass_engine_destroy(rass_engine_t* eng);
int rass_engine_dim(const rass_engine_t* eng);
int rass_engine_device(const rass_engine_t* eng);
/* Run all engine work on a caller-owned hipStream_t (e.g. torch's current
 * stream).  The value is taken literally: NULL is HIP's legacy null stream. */
int rass_engine_set_stream(rass_engine_t* eng, void* stream);
/* Go back to the engine's own (non-blocking) stream. */
int rass_engine_reset_stream(rass_engine_t* eng);
/* The hipStream_t engine work is currently enqueued on. */
void* rass_engine_get_stream(rass_engine_t* eng);
int rass_engine_synchronize(rass_engine_t* eng);

/* ----------------------------------------------------------------- index */

/* Scores that are not finite (DESIGN.md §3 "Scores that are not finite").
 * Nothing refuses a row or a query that holds a NaN or an Inf: normalising a vector with one NaN stores an all-NaN row, one
 * with an Inf stores [0, ..., NaN, ..., 0], and normalize = 0 stores what it is given.  The oracle's rule (oracle/rass_oracle.c,
 * topk_insert) holds for every search form of this header, flat, prefiltered and IVF alike:
 *  - A live row whose score for a query is NaN or -inf is, for that query, as if it were deleted.
 *  - Such a row is never returned, never counted (totals, hits, bucket and group counts), never the representative of a group or
 *    bucket, and never sets the status of a grouped or counted search.
 *  - Such a row is never what fills or displaces a result slot: the other rows of the answer are the ones, and the bits, the
 *    same index gives with that row deleted.
 *  - A query that normalises to NaN gets the empty answer of its entry point: (-inf, -1) lists (-1 groups and ranks), totals,
 *    bucket counts and group counts of 0.  It does not disturb the other queries of its call.
 *  - rass_topk_merge* drop an entry whose score is NaN or -inf whatever its id; +inf ranks first, by id.
 * An IVF keeps such a row in list 0, where no probe finds it; training leaves it out, and no centroid is ever not finite.
 * Out of scope: refusing rows that are not finite at rass_index_add*; rows whose score overflows to +inf; and
 * rass_index_rows_gram called directly on such a row, which keeps its IEEE results. */

/* Replaces ensure_index_exists()'s knn_vector field (app/main.py:350-579,
 * vector field 563-572; name from get_index_name 346-347): look up the named
 * cosine index, creating it when absent.  O(1) when it exists, because the
 * reference constructs OpenSearchIndexer per request (app/main.py:2802). */
int rass_index_open(rass_engine_t* eng, const char* name, rass_dtype dtype,
                    int64_t initial_capacity_rows, rass_index_t** out);
/* Drop an index and free its HBM. */
int rass_index_drop(rass_engine_t* eng, const char* name);
/* Replaces OpenSearchIndexer.has_any_data's count (app/main.py:1470-1478):
 * live (non-deleted) rows. */
int64_t rass_index_count(const rass_index_t* idx);
/* Rows ever appended (live + tombstoned) = next row id. */
int64_t rass_index_rows(const rass_index_t* idx);
int rass_index_dim(const rass_index_t* idx);
int rass_index_row_stride(const rass_index_t* idx); /* elements: dim padded to 128 (dim <= 1024) or to 256 (above) */
/* RASS_F32 / RASS_BF16 as given to rass_index_open (or read back by rass_index_load). */
int rass_index_dtype(const rass_index_t* idx);
/* != 0 once any row carries a caller-assigned GLOBAL id (rass_index_add_ex: a shard of a multi-GPU index).  Together
 * with the dtype and the row count this is what decides whether an index may join a cross-index batch
 * (rass_index_search_multi: fp32, plain row ids, <= 65 536 tiles of 32 rows per batch). */
int rass_index_has_global_ids(const rass_index_t* idx);

/* Replaces the vector half of store_fhir_docs_in_opensearch (app/main.py:
 * 1245-1282: normalise 1249-1251 + bulk index).  Appends n rows of `dim`
 * floats (host memory).  When `normalize` != 0 rows are L2-normalised on the
 * GPU with the reference's formula e / (||e|| + 1e-9).  `tags` (may be NULL =
 * all 0) is one int32 per row: the dictionary code of the row's patientId
 * (the reference's `_routing` / term-filter key, app/main.py:1263, 1549);
 * must be >= 0.  Row ids are insertion ordinals; *first_row receives the id of
 * the first appended row.  Append-only: overwrite = rass_index_delete + add. */
int rass_index_add(rass_index_t* idx, const float* vecs, const int32_t* tags,
                   int64_t n, int normalize, int64_t* first_row);
/* Same, from device memory (the encoder's pooled output), async on the
 * engine stream.  Device tags cannot be validated without a sync: negative values are stored as
 * 0 (the tombstone code belongs to rass_index_delete). */
int rass_index_add_device(rass_index_t* idx, const float* d_vecs,
                          const int32_t* d_tags, int64_t n, int normalize,
                          int64_t* first_row);
/* Append with CALLER-ASSIGNED ids: row i of the batch is reported by searches as
 * first_global_id + i instead of its ordinal (first_global_id = -1: ordinals, as rass_index_add).
 * This is what makes an index one SHARD of a multi-GPU index whose batches are dealt round-robin to
 * the ranks (rassengine_amd/serving.py; the reference's analogue is OpenSearch routing docs to
 * SHARD_COUNT shards, app/main.py:89, 357): ids must ascend with the append order, so the per-shard
 * (score desc, id asc) order is the global one and the cross-shard merge reproduces the single-index
 * result.  rass_index_delete / get_row(s) keep addressing rows by ORDINAL (*first_row); the caller
 * maps global ids to (rank, ordinal).  `device_source` != 0: vecs / tags are device pointers.
 * On such an index id_base is ignored, k <= RASS_MAX_K, and the prefilter mode is not used. */
int rass_index_add_ex(rass_index_t* idx, const float* vecs, const int32_t* tags,
                      int64_t n, int normalize, int64_t first_global_id,
                      int device_source, int64_t* first_row);
/* Tombstone a row (the overwrite semantics of `_id=doc_id`, app/main.py:1260). */
int rass_index_delete(rass_index_t* idx, int64_t row);
/* Remove every tombstoned row: live rows keep their relative order and their stored bits and take the
 * ordinals 0 .. live-1; rass_index_rows() == rass_index_count() afterwards.  new_row_of (host, may be NULL)
 * receives, for each of the *rows_before old ordinals, the new ordinal or -1; map_capacity < rows ->
 * RASS_ERR_INVALID and nothing changes.  Caller-assigned ids (rass_index_add_ex) travel with their rows.
 * Out of place: needs HBM for the compacted index next to the old one; RASS_ERR_OOM leaves the index as it was.
 * No tombstone -> RASS_OK, identity map, nothing moved, layout epoch unchanged.
 * fp32 indices in every prefilter mode (the candidate copies are rebuilt from the moved rows; mode 3's
 * certificate maxima and counters are kept) and bf16 indices.  The HBM the index holds afterwards is that of
 * its live rows (at least 1 024).  An IVF built from the index names its old ordinals: rebuild it. */
int rass_index_compact(rass_index_t* idx, int64_t* new_row_of, int64_t map_capacity,
                       int64_t* rows_before, int64_t* rows_after);
/* Number of compactions that moved rows: a row ordinal is only meaningful together with this value.
 * The host search entry points (rass_index_search, _ex, _multi) answer from ONE layout: read the epoch
 * before and after such a call, and where the two agree the ids are ordinals of that layout.  The device
 * entry points are asynchronous: pair their ids with the epoch read before the call.  0 after open / load. */
int64_t rass_index_layout_epoch(const rass_index_t* idx);
/* Copy one stored (normalised) row back to the host as fp32 (dim floats): the
 * reference returns the embedding inside `_source` (app/main.py:1555-1557). */
int rass_index_get_row(rass_index_t* idx, int64_t row, float* out);
/* Same for rows [first_row, first_row + n): n x dim floats, row-major. */
int rass_index_get_rows(rass_index_t* idx, int64_t first_row, int64_t n,
                        float* out);

/* Replaces the knn query of OpenSearchIndexer.semantic_search (app/main.py:
 * 1527-1560) and the knn sub-clauses of hybrid_search (1595),
 * hybrid_structured_search (1754), multi_intent_search (2003): exact cosine
 * top-k.  `queries` is nq x dim fp32 (host); they are re-normalised on the
 * GPU exactly as the reference does (1536-1537).  `q_filter` (may be NULL) is
 * one int32 per query: RASS_QFILTER_NONE or the patientId code to restrict to
 * (the `term: patientId` filter, 1549), applied as a pre-filter.
 * Outputs: out_scores[nq*k] raw cosine, best first; out_ids[nq*k] global row
 * ids (id_base + local row), -1 (score -inf) where fewer than k rows match.
 * Order: score descending, ties by id ascending.  1 <= k <= RASS_MAX_K; any nq
 * (scanned in batches of RASS_MAX_QBATCH). */
int rass_index_search(rass_index_t* idx, const float* queries, int nq, int k,
                      const int32_t* q_filter, float* out_scores,
                      int64_t* out_ids);
/* Extended host search.  (1) `q_filter_mask` (may be NULL = exact compare): a row matches query q
 * when (row_tag & q_filter_mask[q]) == q_filter[q], so one compare serves `term: patientId`
 * (app/main.py:1549), the `term: doc_type` of hybrid_structured_search (app/main.py:1765) or both.
 * (2) 1 <= k <= RASS_MAX_K_MULTIPASS: the reference passes the caller's top_k straight through
 * (app/main.py:2882, 3008); k > RASS_MAX_K is served exactly, in ceil(k/32) passes, pass p ranking only
 * the rows strictly after pass p-1's last hit under (score desc, id asc).
 * Thread-safe: concurrent calls (same or different indices) overlap their host round trips; the
 * engine lock is held while enqueuing only. */
int rass_index_search_ex(rass_index_t* idx, const float* queries, int nq, int k,
                         const int32_t* q_filter, const int32_t* q_filter_mask,
                         float* out_scores, int64_t* out_ids);
/* CROSS-INDEX batch: query i is answered over index idxs[i] (the reference keeps one index per user,
 * app/main.py:346-347, and serves users concurrently: their queries then share ONE scan launch instead of one
 * launch per user).  All indices must live on one engine, be fp32 and carry plain row ids; any nq (groups of 32).
 * Each distinct index of a group is streamed once, whatever the number of its queries; out_ids are rows of the
 * query's own index.  A group may cover at most 65 536 32-row tiles (2 M rows) over its distinct indices. */
int rass_index_search_multi(rass_index_t* const* idxs, const float* queries, int nq, int k,
                            const int32_t* q_filter, const int32_t* q_filter_mask,
                            float* out_scores, int64_t* out_ids);
/* Device-resident variant for the multi-GPU path and the benchmark: queries
 * and outputs live in HBM, nothing is synchronised; nq <= RASS_MAX_QBATCH.
 * `id_base` is added to local row ids (row-sharded corpus). */
int rass_index_search_device(rass_index_t* idx, const float* d_queries, int nq,
                             int k, const int32_t* d_q_filter, int64_t id_base,
                             float* d_out_scores, int64_t* d_out_ids);

/* Same with the masked filter of rass_index_search_ex ((tag & mask) == filter); on an index
 * with caller-assigned ids (rass_index_add_ex) those ids are reported and id_base is ignored. */
int rass_index_search_device_ex(rass_index_t* idx, const float* d_queries,
                                int nq, int k, const int32_t* d_q_filter,
                                const int32_t* d_q_filter_mask, int64_t id_base,
                                float* d_out_scores, int64_t* d_out_ids);

/* One pass of a k > RASS_MAX_K search over a SHARD (rassengine_amd/serving.py): query q ranks only the rows strictly
 * after (d_after_score[q], row d_after_row[q]) in (score desc, row asc) order, i.e. score < after_score, or equal
 * and row ordinal > after_row (-1: every tying row counts).  A multi-GPU front asks every shard for its next 32
 * behind the previous pass's last GLOBAL hit — each rank translates that hit's id into its own row ordinals, which
 * ascend with the ids — and merges; the reference passes the caller's top_k straight through (app/main.py:2882,
 * 3008).  Reported ids are the index's own (caller-assigned ids where rass_index_add_ex gave them, else ordinals);
 * the bound's row and the tie order are always in row ORDINALS.
 * The bound need not be a row's own score, and after_row may be ANY int64: it need not name a live row, a row the
 * query's filter lets through, or a row at all (-1, or a value at or past the row count: no row tying with
 * after_score counts).  after_score = +inf: every row ranks (the plain top-k, whatever after_row is); -inf: none;
 * NaN: none either (both comparisons above are false for every score).  The bound is honoured exactly whatever the
 * prefilter mode (a bounded request always takes the exact scan) and on RASS_BF16 indices.  1 <= nq <=
 * RASS_MAX_QBATCH, 1 <= k <= RASS_MAX_K; fewer than k rows behind the bound: (-inf, -1) past the end.
 * (tests/test_gpu_search_after.py holds all of this to the CPU oracle.) */
int rass_index_search_device_after(rass_index_t* idx, const float* d_queries, int nq, int k,
                                   const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                   const float* d_after_score, const int64_t* d_after_row,
                                   float* d_out_scores, int64_t* d_out_ids);

/* Many launch groups in one call (nq <= RASS_MAX_DEVICE_BATCH, k <= RASS_MAX_K): the result is, bit for bit,
 * that of rass_index_search_device on consecutive groups of RASS_MAX_QBATCH queries, but on an fp32 index the
 * batch shares ONE normalise launch and ONE merge launch and runs the groups' score-floor sample passes back to
 * back ahead of the big scans, so the serial tail a lone group pays after its scan is paid once.
 * Consecutive full groups are scanned two per corpus pass (64 queries per launch; RASS_SCAN_BATCH_PAIR=0: one launch per group).
 * This is the shape of the reference's load: embed_texts_in_batches / ask() under concurrent users hand the
 * engine many queries at once (app/main.py:1536-1560 is called per request; the micro-batcher coalesces them).
 * Group g's results go to d_out_scores + g * out_scores_group_stride (floats) and d_out_ids + g *
 * out_ids_group_stride (int64s); 0 = contiguous [nq][k].  d_q_filter: nq tags or NULL. */
int rass_index_search_device_batch(rass_index_t* idx, const float* d_queries, int nq, int k,
                                   const int32_t* d_q_filter, int64_t id_base,
                                   float* d_out_scores, int64_t* d_out_ids,
                                   int64_t out_scores_group_stride, int64_t out_ids_group_stride);

/* Score-threshold (RADIAL) search: every row whose score is at least min_score[q] — the radial form of the k-NN clause
 * (`min_score` instead of `k`) — and how many there are, in ONE corpus pass per launch group: the flat scan computes every
 * (row, query) score anyway, and a threshold question needs no ranking inside it, only emission.
 * A row MATCHES query q when it is live, passes the filter exactly as in rass_index_search_ex (q_filter NULL, exact, or
 * (tag & q_filter_mask[q]) == q_filter[q]) and its score s satisfies s >= min_score[q].  s is the fp32 value of the flat
 * scan (the same MFMA chain, the same p0 + ... + p7 sum of the partials): bit-identical to the score rass_index_search_ex
 * reports for that row.  out_total[q] is the EXACT number of matching rows, whatever max_hits is.
 * out_scores / out_ids are [nq][max_hits], 1 <= max_hits <= RASS_MAX_K_MULTIPASS: the matching rows, score descending, ties
 * by id ascending, (-inf, -1) past the end.  Ids as rass_index_search_ex reports them: ordinals, or the caller-assigned ids
 * of rass_index_add_ex.
 * More matches than max_hits (out_total[q] > max_hits): the list holds the BEST max_hits matching rows, which the call
 * gets from the exact k = max_hits path of rass_index_search_ex for those queries only (ceil(max_hits / 32) more passes;
 * on an index with caller-assigned ids that path serves max_hits <= RASS_MAX_K, beyond: RASS_ERR_UNSUPPORTED).
 * min_score: -inf is allowed (with a patient filter out_total is then that patient's live row count); NaN ->
 * RASS_ERR_INVALID.  Any nq (scanned in groups of RASS_MAX_QBATCH).
 * fp32 indices of every dim the engine takes, wide rows included; a bf16 index answers RASS_ERR_UNSUPPORTED.  The
 * prefilter mode of the index is ignored: a range search always runs the exact scan, because a candidate scan cannot
 * bound a count.  IVF, cross-index batches and the sharded multi-GPU front have no range form.
 * Thread-safety and layout epochs as rass_index_search_ex: the engine lock is held while enqueuing only, and the answer
 * comes from ONE layout of the index. */
int rass_index_search_range(rass_index_t* idx, const float* queries, int nq,
                            const float* min_score, int max_hits,
                            const int32_t* q_filter, const int32_t* q_filter_mask,
                            float* out_scores, int64_t* out_ids, int64_t* out_total);
/* Device-resident variant: every pointer is device memory, nothing is synchronised and nothing is read back;
 * nq <= RASS_MAX_QBATCH.  Ids are id_base + row (ignored on an index with caller-assigned ids, which are reported), to be
 * paired with the layout epoch read before the call.  d_total[q] is the exact count as above.  A query with more matches
 * than max_hits gets the EMPTY list (every slot (-inf, -1)) and d_total[q] says why: which max_hits of the matching rows
 * the scan kept depends on the order its workgroups ran in, so they are not reported; ask again with a larger max_hits,
 * a higher threshold, or rass_index_search_device_ex with k = max_hits.  A NaN threshold matches nothing (total 0): it
 * cannot be refused without reading it back. */
int rass_index_search_range_device(rass_index_t* idx, const float* d_queries, int nq,
                                   const float* d_min_score, int max_hits,
                                   const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                   int64_t id_base, float* d_out_scores, int64_t* d_out_ids,
                                   int64_t* d_total);

/* Grouped (COLLAPSED) search: the best row of every group, the k best groups — OpenSearch's `"collapse": {"field": ...}` next to
 * a k-NN clause.  The group of a row is a bit field of its tag: (tag & group_mask) >> ctz(group_mask); RASS_TAG_PATIENT_MASK
 * collapses by patient, RASS_TAG_DOCTYPE_MASK by doc type.  Group 0 ("none") is a group like any other, as OpenSearch
 * collapses missing values together.  ONE corpus pass per launch group answers any k exactly: the flat scan keeps a running
 * maximum per (query, group) instead of ranking rows, and a select over the n_groups slots of each query finishes it.
 * A row MATCHES query q exactly as in rass_index_search_ex: it is live and passes q_filter (NULL, exact, or
 * (tag & q_filter_mask[q]) == q_filter[q]).  Every group with a matching row is REPRESENTED by its best matching row under
 * (score descending, row ordinal ascending); the answer lists the representatives of the k best groups in that same order:
 * out_scores / out_ids / out_groups are [nq][k], (-inf, -1, -1) past the end.  Scores are the fp32 values of the flat scan (the
 * same MFMA chain, the same p0 + ... + p7 sum): bit-identical to what rass_index_search_ex reports for that row.  Ids as
 * rass_index_search_ex reports them: ordinals, or the caller-assigned ids of rass_index_add_ex.  out_group_total[q] is the
 * EXACT number of distinct groups with a matching row, whatever k is.
 * group_mask: non-zero, within 0x7fffffff.  n_groups: the exclusive bound of the group key, 1 .. 1 048 576 (the call keeps
 * nq x n_groups 8-byte slots on the device, up to 256 MiB, in an engine-owned block grown on demand; RASS_ERR_OOM when it
 * cannot be had, and nothing has changed).  1 <= k <= RASS_MAX_K_MULTIPASS.  Outside those: RASS_ERR_INVALID.
 * A live matching row whose group key is >= n_groups is left out of the answer: RASS_ERR_INVALID, named in
 * rass_last_error(), and the outputs are unspecified.  Any nq (scanned in groups of RASS_MAX_QBATCH).
 * fp32 indices of every dim the engine takes, wide rows included; a bf16 index answers RASS_ERR_UNSUPPORTED.  The
 * prefilter mode of the index is ignored: a candidate scan cannot see a group's maximum.  IVF, cross-index batches
 * (rass_index_search_multi), the sharded multi-GPU front and the 64-query pair kernel of the batch call have no grouped form.
 * Thread-safety and layout epochs as rass_index_search_range: the engine lock is held while enqueuing only, and the answer
 * comes from ONE layout of the index. */
int rass_index_search_grouped(rass_index_t* idx, const float* queries, int nq, int k,
                              int32_t group_mask, int32_t n_groups,
                              const int32_t* q_filter, const int32_t* q_filter_mask,
                              float* out_scores, int64_t* out_ids, int32_t* out_groups,
                              int64_t* out_group_total);
/* Device-resident variant: every pointer is device memory, the call is stream-ordered, nothing is synchronised and nothing is
 * read back; nq <= RASS_MAX_QBATCH.  Ids are id_base + row (ignored on an index with caller-assigned ids, which are
 * reported), to be paired with the layout epoch read before the call.  *d_status = 1 when a live matching row's group key was
 * >= n_groups (that row is left out; the other rows' answer is intact), else 0. */
int rass_index_search_grouped_device(rass_index_t* idx, const float* d_queries, int nq, int k,
                                     int32_t group_mask, int32_t n_groups,
                                     const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                     int64_t id_base, float* d_out_scores, int64_t* d_out_ids,
                                     int32_t* d_out_groups, int64_t* d_group_total, int32_t* d_status);

/* ALLOW-LIST search: the exact top-k among the rows a per-query BITMAP allows — the general restriction next to the tag
 * compare: a set of patients or doc types (OpenSearch `terms`), the hit set of a text query (`ids`), an ACL resolved
 * elsewhere, or a predicate over the index's attribute columns (rass_index_allow_from_attr_clauses: `term`, `range`).  A bitmap is uint32 words, bit (r & 31) of word r >> 5 allows row ordinal r; `allow` is
 * uint32[n_bitmaps][words_per_bitmap], row-major, words_per_bitmap >= ceil(rows / 32) for the index's row count at the call.
 * n_bitmaps = nq: bitmap q belongs to query q; n_bitmaps = 1: ONE bitmap shared by every query (it is read in place, never
 * expanded).  Bits of tombstoned rows, bits at or past the row count and surplus words allow nothing.
 * A row MATCHES query q when it is live, passes the filter exactly as in rass_index_search_ex (q_filter NULL, exact, or
 * (tag & q_filter_mask[q]) == q_filter[q]) and its bit is set.  out_scores / out_ids are [nq][k]: the matching rows, score
 * descending, ties by row ordinal ascending, (-inf, -1) past the end, as rass_index_search_ex pads.  Scores are the fp32
 * values of the flat scan (the same MFMA chain, the same p0 + ... + p7 sum): bit-identical to what rass_index_search_ex
 * reports for that row; with every bit set the answer IS rass_index_search_ex's.  Ids as rass_index_search_ex reports them:
 * ordinals, or the caller-assigned ids of rass_index_add_ex.
 * Cost follows the bitmap, not the index: per launch group of RASS_MAX_QBATCH queries a plan kernel lists the 32-row tiles
 * in which some query has a bit set, and the scan streams those tiles only.  No sample floor is used.
 * 1 <= k <= RASS_MAX_K_MULTIPASS (k > RASS_MAX_K in passes of RASS_MAX_K under the continuation bound, over the same work
 * list); 0 <= nq <= RASS_MAX_DEVICE_BATCH.  Outside those, n_bitmaps neither 1 nor nq, or words_per_bitmap too small:
 * RASS_ERR_INVALID.  fp32 indices with dim <= 1024; a bf16 index or a wide-row index answers RASS_ERR_UNSUPPORTED.  The
 * prefilter mode of the index is ignored: an allowed search always runs the exact fp32 scan.  (An IVF over the index takes
 * the same bitmaps in rass_ivf_search_allowed_delta.)  Cross-index batches
 * (rass_index_search_multi), the sharded multi-GPU front, the 64-query pair kernel and the range search have no allow-list
 * form; the grouped search and the aggregation take a bitmap in their key-column forms (rass_index_search_grouped_keys,
 * rass_index_aggregate_keys), which stream every tile.
 * A bitmap names row ordinals of ONE layout of the index: build it and search under one layout epoch
 * (rass_index_layout_epoch).  Thread-safety and layout epochs as rass_index_search_ex. */
int rass_index_search_allowed(rass_index_t* idx, const float* queries, int nq, int k,
                              const uint32_t* allow, int n_bitmaps, int64_t words_per_bitmap,
                              const int32_t* q_filter, const int32_t* q_filter_mask,
                              float* out_scores, int64_t* out_ids);
/* Device-resident variant: every pointer is device memory, the call is stream-ordered, nothing is synchronised and nothing
 * is read back; the same bounds on nq and k (every pass of a k > RASS_MAX_K search is enqueued by the one call).  Ids are
 * id_base + row (ignored on an index with caller-assigned ids, which are reported). */
int rass_index_search_allowed_device(rass_index_t* idx, const float* d_queries, int nq, int k,
                                     const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                     const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                     int64_t id_base, float* d_out_scores, int64_t* d_out_ids);
/* Bitmap builders: d_allow is DEVICE memory of `words` >= ceil(rows / 32) uint32, overwritten whole; rows / values are HOST
 * arrays.  Stream-ordered on the engine's stream; the host arrays may be reused when the call returns.
 * _from_rows: the bits of the n row ordinals in `rows`; ids outside [0, rows) are ignored, duplicates are fine.
 * _from_tag_values: the bit of every live row whose (tag & mask) is one of the n_values `values` (any order, duplicates
 * fine): OpenSearch's `terms` filter on patientId (mask RASS_TAG_PATIENT_MASK) or doc_type (RASS_TAG_DOCTYPE_MASK, values
 * shifted by RASS_TAG_DOCTYPE_SHIFT). */
int rass_index_allow_from_rows(rass_index_t* idx, const int64_t* rows, int64_t n, uint32_t* d_allow, int64_t words);
int rass_index_allow_from_tag_values(rass_index_t* idx, const int32_t* values, int64_t n_values, int32_t mask,
                                     uint32_t* d_allow, int64_t words);
/* The work list an allowed search of ONE launch group (1 <= nq <= RASS_MAX_QBATCH) would walk, for tests and tools: d_allow
 * as in rass_index_search_allowed_device.  *out_n = the number of items = the tiles in which some query has a bit set below
 * the row count; the first min(*out_n, capacity) items, tiles ascending, go to the HOST arrays out_tile / out_rows (rows of
 * the tile that exist) / out_mask (bit q set iff query q has a bit set in the tile).  Synchronises. */
int rass_index_allow_plan(rass_index_t* idx, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap, int nq,
                          int32_t* out_tile, int32_t* out_rows, uint32_t* out_mask, int64_t capacity, int64_t* out_n);
/* out_counts[b] (HOST int64, 1 <= n_bitmaps <= RASS_MAX_DEVICE_BATCH of them) = the bits bitmap b has set below the index's
 * row count: how many rows it names, tombstoned ones included — what a caller weighs an exact allowed search against an IVF
 * probe within the bitmap by (rass_ivf_search_allowed_delta).  d_allow as in rass_index_search_allowed_device.  Synchronises. */
int rass_index_allow_count(rass_index_t* idx, const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                           int64_t* out_counts);

/* ATTRIBUTE COLUMNS: up to RASS_MAX_ATTRS typed per-row fields next to the tag — a keyword's dictionary code, an integer, a
 * date as days since 1970-01-01 — for the stored-field filters OpenSearch takes next to a k-NN clause (`term`, `terms`,
 * `range`, `exists`).  Column c is int32[capacity] in HBM, allocated by the first rass_index_set_attr on it and filled with
 * RASS_ATTR_MISSING; an index on which no column was ever set allocates nothing, reads nothing and saves today's bytes.
 * Valid values are every int32 above RASS_ATTR_MISSING; storing RASS_ATTR_MISSING un-sets a value.  fp32, bf16 and wide-row
 * indices all take columns (only the allow-list search refuses the latter two, as before).
 * ORDERING: a row appended by any rass_index_add* (or rass_index_fill_synthetic) reads RASS_ATTR_MISSING in every allocated
 * column until rass_index_set_attr names it: until then no non-negated clause matches it.  Add, then set, then tombstone what
 * the rows replace.  The columns follow their rows through growth, rass_index_compact (new ordinals), save and load (a
 * second flag bit in the file header and a section after the ids; files without columns are unchanged and old files load);
 * rass_index_delete leaves the values alone: the tombstone in the tag is what counts.
 * _set_attr: `values` is a HOST array of n int32 for rows [first_row, first_row + n), which must lie within the rows at the
 *   call; stream-ordered on the engine's stream, the array may be reused on return.  col outside 0 .. RASS_MAX_ATTRS - 1, a
 *   range outside the rows, or NULL with n > 0: RASS_ERR_INVALID.
 * _get_attr: the values of rows [first_row, first_row + n) to the HOST array `out`; synchronises.  A column that was never
 *   set reads as all RASS_ATTR_MISSING.
 * _attr_mask: bit c set iff column c is allocated.  _device_attr: the device pointer of column c (as rass_index_device_tags;
 *   invalidated by growth and compaction), NULL for a column that was never set. */
int rass_index_set_attr(rass_index_t* idx, int col, int64_t first_row, int64_t n, const int32_t* values);
int rass_index_get_attr(rass_index_t* idx, int col, int64_t first_row, int64_t n, int32_t* out);
int rass_index_attr_mask(const rass_index_t* idx);
void* rass_index_device_attr(rass_index_t* idx, int col);
/* PREDICATES -> BITMAPS: the builder that turns clauses over the columns into the bitmaps rass_index_search_allowed(_device)
 * consumes.  `clauses` is a HOST array int32[n_clauses][5] = {query, col, lo, hi, negate}.  A clause HOLDS for a row whose
 * value in `col` is v when v != RASS_ATTR_MISSING && lo <= v && v <= hi; with negate != 0 the result is inverted, so a
 * missing value passes a negated clause (OpenSearch's must_not over an absent field).  lo > hi holds for nothing; `exists`
 * is [INT32_MIN + 1, INT32_MAX]; equality is lo == hi; a column that was never set is all-missing.
 * mode RASS_ATTR_ALL: query q allows a LIVE row iff all of q's clauses hold (no clause: every live row); RASS_ATTR_ANY: iff
 * at least one holds (no clause: no row).  combine says how the result meets what d_allow already holds — RASS_ATTR_REPLACE,
 * _AND, _OR — so a formula composes by successive calls, and with rass_index_allow_from_rows / _from_tag_values, which
 * overwrite: run those first, then refine with _AND.  d_allow is DEVICE memory uint32[n_bitmaps][words_per_bitmap],
 * words_per_bitmap >= ceil(rows / 32); n_bitmaps = nq, or 1 for one shared bitmap, whose clauses must all name query 0.
 * Tombstoned rows never get a bit.  Bits at or past the row count and surplus words come out 0 under _REPLACE and _AND and
 * are left as they were under _OR.  1 <= nq <= RASS_MAX_DEVICE_BATCH (launch groups of RASS_MAX_QBATCH queries: one pass
 * over the named columns and the tags per group), at most RASS_MAX_ATTR_CLAUSES clauses per query per call; anything outside
 * those bounds: RASS_ERR_INVALID with the reason in rass_last_error().  Stream-ordered on the engine's stream; the host
 * array may be reused when the call returns.  A bitmap names rows of ONE layout epoch, as every bitmap does. */
int rass_index_allow_from_attr_clauses(rass_index_t* idx, const int32_t* clauses, int64_t n_clauses, int nq, int n_bitmaps,
                                       int mode, int combine, uint32_t* d_allow, int64_t words_per_bitmap);
/* Word-wise merge of two DEVICE bitmaps of `words` uint32 each, for the formulas one builder call cannot fold (two nested
 * sub-formulas under one and / or, a negated tag-value set): d_dst = d_dst & d_src (RASS_ATTR_AND), | d_src (RASS_ATTR_OR)
 * or & ~d_src (RASS_ATTR_ANDNOT; "not x" is the all-live bitmap — an RASS_ATTR_ALL call without clauses — and-not x).  `words`
 * may span several bitmaps laid out alike.  d_dst and d_src must not overlap.  Stream-ordered on the engine's stream. */
int rass_index_allow_combine(rass_index_t* idx, uint32_t* d_dst, const uint32_t* d_src, int64_t words, int op);

/* BOOSTED search: the exact top-k of
 *     fused = boost[q] * T(cos) + bonus[q][row]
 * over a flat index — an OpenSearch bool.should around a knn clause: the knn clause's boost, and per row the sum of what the
 * other matching clauses are worth (text hits, recency ranges, per-document priors, decay), whatever their number or sign.
 * The bonus is a dense fp32 COLUMN in device memory, d_bonus = float[n_bonus][bonus_stride]: n_bonus = nq (column q belongs to
 * query q) or 1 (ONE column shared by every query, read in place).  Rows at or past bonus_rows (<= bonus_stride) read 0, so
 * rows appended after a column was built carry no bonus.  boost: HOST float[nq], or NULL = 1.0 for every query; every value
 * must be finite (negative, zero and fractional boosts are fine).  transform RASS_BOOST_RAW: T(s) = s; RASS_BOOST_OPENSEARCH:
 * T(s) = 1 / (2 - s), the k-NN plugin's cosinesimil score.
 * ARITHMETIC, all fp32: s is the flat scan's cosine, bit for bit what rass_index_search_ex reports for the row; T's
 * subtraction and division, the product boost * T and the sum with the bonus are each ONE correctly rounded operation, in that
 * order, never contracted into an fma.
 * A row RANKS for query q when it is live, passes the filter exactly as in rass_index_search_ex, has s > -inf (the rule under
 * "Scores that are not finite": a NaN or -inf cosine drops the row whatever its bonus) and has fused > -inf — so a bonus of
 * -inf or NaN EXCLUDES the row, which is how a row bitmap composes with the column (rass_index_bonus_mask).  +inf is out of
 * scope, as everywhere.  out_scores / out_ids are [nq][k]: fused descending, ties by row ordinal ascending, (-inf, -1) past
 * the end; ids as rass_index_search_ex reports them.
 * One corpus pass per launch group of RASS_MAX_QBATCH queries whatever the column holds; every tile is streamed; no sample
 * floor (a floor is only valid under the score it was sampled with).  1 <= k <= RASS_MAX_K_MULTIPASS (k > RASS_MAX_K in passes
 * of RASS_MAX_K chained on the device under the continuation bound, taken on the fused score); 0 <= nq <=
 * RASS_MAX_DEVICE_BATCH.  Outside those, n_bonus neither 1 nor nq, bonus_rows outside [0, bonus_stride], a non-finite boost, an
 * unknown transform, or a launch group whose columns span 2 GiB or more: RASS_ERR_INVALID, nothing is launched and the outputs
 * are untouched.  fp32 indices with dim <= 1024: a bf16 index or a wide-row index answers RASS_ERR_UNSUPPORTED.  The prefilter
 * mode is ignored.  IVF probes, cross-index batches and the sharded front have no boosted form.
 * A column names row ordinals of ONE layout of the index (rass_index_layout_epoch).  Thread-safety as rass_index_search_ex. */
#define RASS_BOOST_RAW 0
#define RASS_BOOST_OPENSEARCH 1
int rass_index_search_boosted(rass_index_t* idx, const float* queries, int nq, int k,
                              const float* boost, int transform,
                              const float* d_bonus, int n_bonus, int64_t bonus_rows, int64_t bonus_stride,
                              const int32_t* q_filter, const int32_t* q_filter_mask,
                              float* out_scores, int64_t* out_ids);
/* Device-resident variant: every pointer is device memory (d_boost too; its values are the caller's to keep finite), the call
 * is stream-ordered, nothing is synchronised and nothing is read back; every pass of a k > RASS_MAX_K search is enqueued by
 * the one call.  Ids are id_base + row (ignored on an index with caller-assigned ids, which are reported). */
int rass_index_search_boosted_device(rass_index_t* idx, const float* d_queries, int nq, int k,
                                     const float* d_boost, int transform,
                                     const float* d_bonus, int n_bonus, int64_t bonus_rows, int64_t bonus_stride,
                                     const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                     int64_t id_base, float* d_out_scores, int64_t* d_out_ids);
/* COLUMN BUILDERS.  They work on a caller-owned DEVICE block d_bonus = float[n_bonus][stride], stride a multiple of 32 and >=
 * the index's rows at the call, 1 <= n_bonus <= RASS_MAX_DEVICE_BATCH.  Zero-filling is the caller's (hipMemsetAsync on the
 * engine's stream).  Every value is built from separately rounded fp32 adds in a stated order: a host restatement reproduces a
 * column word for word.  All are stream-ordered on the engine's stream; host arrays may be reused when a call returns.
 * _scatter: bonus[q_of[i]][rows[i]] += values[i] for the n HOST triples.  The (column, row) pairs must be unique within a call:
 *   duplicates, a column outside [0, n_bonus) or a row outside [0, rows) are RASS_ERR_INVALID and nothing is written (sum
 *   duplicates first).  _scatter_device takes DEVICE arrays and checks nothing of their contents: uniqueness and range are the
 *   caller's duty (each cell has one writer; no atomics).
 * _from_attr_clauses: weighted predicates over the attribute columns.  `clauses` is a HOST array int32[n_clauses][5] = {query,
 *   col, lo, hi, negate} with rass_index_allow_from_attr_clauses' semantics, RASS_ATTR_MISSING included; weights[i] is clause
 *   i's fp32 weight.  Per (query, row): b = 0 (op RASS_BONUS_REPLACE) or the cell's value (RASS_BONUS_ADD), then b = b +
 *   weight for every clause of that query that holds, in LIST order.  n_bonus = nq, or 1 for a shared column whose clauses all
 *   name query 0; at most RASS_MAX_ATTR_CLAUSES clauses per query per call.  Rows [0, rows) of every column are written,
 *   tombstoned rows too (they never rank); cells at or past the row count are left alone.
 * _mask: bonus[q][r] = -inf where bit r of bitmap q is clear (d_allow = uint32[n_bitmaps][words] as
 *   rass_index_search_allowed_device takes it, n_bitmaps = n_bonus or 1, words >= ceil(rows / 32)): a `where` filter inside a
 *   boosted search, without another scan mode. */
#define RASS_BONUS_REPLACE 0
#define RASS_BONUS_ADD 1
int rass_index_bonus_scatter(rass_index_t* idx, const int32_t* q_of, const int64_t* rows, const float* values, int64_t n,
                             float* d_bonus, int n_bonus, int64_t stride);
int rass_index_bonus_scatter_device(rass_index_t* idx, const int32_t* d_q_of, const int64_t* d_rows, const float* d_values,
                                    int64_t n, float* d_bonus, int n_bonus, int64_t stride);
int rass_index_bonus_from_attr_clauses(rass_index_t* idx, const int32_t* clauses, const float* weights, int64_t n_clauses,
                                       int nq, int n_bonus, float* d_bonus, int64_t stride, int op);
int rass_index_bonus_mask(rass_index_t* idx, float* d_bonus, int n_bonus, int64_t stride, const uint32_t* d_allow,
                          int n_bitmaps, int64_t words);

/* FUNCTION-SCORE search: the exact top-k of
 *     t = T(cos),  a = boost[q] * t,  fused = combine(a, f[q][row])
 * over a flat index — an OpenSearch function_score around a knn clause.  f is a dense fp32 FUNCTION COLUMN in device memory,
 * d_fn = float[n_fn][fn_stride] with the layout and ownership of a bonus block: n_fn = nq (column q belongs to query q) or 1
 * (ONE column shared by every query).  The column must cover EVERY row of the index at the call: fn_rows must equal the
 * index's rows (live and tombstoned), else RASS_ERR_INVALID — "rows past the column read 0" has no meaning that holds in
 * every mode.  boost, transform: as in rass_index_search_boosted.  combine is OpenSearch's boost_mode:
 *     RASS_COMBINE_SUM a + f | _MULTIPLY a * f | _AVG (a + f) * 0.5f | _MAX f > a ? f : a | _MIN f < a ? f : a | _REPLACE f
 * ARITHMETIC, all fp32: the cosine is the flat scan's, bit for bit; T, the product boost * t and every operation of the
 * combine (avg: a rounded add, then a rounded product) are each ONE correctly rounded operation, never contracted into an
 * fma; max and min are a compare and a select (which of two zeros of different sign is reported is thereby fixed).
 * min_score: HOST float[nq], or NULL: the knn clause's radial min_score.  A row ranks for query q only with t >=
 * min_score[q] — the gate is on the TRANSFORMED similarity, before the boost; -inf: no gate; a NaN: RASS_ERR_INVALID.
 * A row RANKS for query q when it is live, passes the filter as in rass_index_search_ex, passes the gate, has cos > -inf, has
 * f > -inf and has fused > -inf.  A NaN or -inf cell of the column EXCLUDES the row in EVERY mode, _MAX and _REPLACE
 * included: rass_index_bonus_mask works on a function column as on a bonus column.  out_scores / out_ids are [nq][k]: fused
 * descending, ties by row ordinal ascending, (-inf, -1) past the end; ids as rass_index_search_ex reports them.
 * One corpus pass per launch group of RASS_MAX_QBATCH queries; every tile is streamed; no sample floor.  1 <= k <=
 * RASS_MAX_K_MULTIPASS (k > RASS_MAX_K in passes of RASS_MAX_K chained on the device under the continuation bound, taken on
 * the fused score); 0 <= nq <= RASS_MAX_DEVICE_BATCH.  Outside those, n_fn neither 1 nor nq, fn_rows outside [0, fn_stride]
 * or not the index's rows, a non-finite boost, a NaN min_score, an unknown transform or combine, or a launch group whose
 * columns span 2 GiB or more: RASS_ERR_INVALID, nothing is launched and the outputs are untouched.  Where the boosted search
 * answers RASS_ERR_UNSUPPORTED (a bf16 index, a wide-row index) so does this one; IVF probes, cross-index batches and the
 * sharded front have no function-score form.  A column names row ordinals of ONE layout.  Thread-safety as
 * rass_index_search_ex. */
#define RASS_COMBINE_SUM 0
#define RASS_COMBINE_MULTIPLY 1
#define RASS_COMBINE_AVG 2
#define RASS_COMBINE_MAX 3
#define RASS_COMBINE_MIN 4
#define RASS_COMBINE_REPLACE 5
int rass_index_search_scored(rass_index_t* idx, const float* queries, int nq, int k,
                             const float* boost, int transform, int combine, const float* min_score,
                             const float* d_fn, int n_fn, int64_t fn_rows, int64_t fn_stride,
                             const int32_t* q_filter, const int32_t* q_filter_mask,
                             float* out_scores, int64_t* out_ids);
/* Device-resident variant: every pointer is device memory (d_boost and d_min_score too; keeping the boosts finite is the
 * caller's; a NaN gate passes no row), the call is stream-ordered, nothing is synchronised and nothing is read back; every
 * pass of a k > RASS_MAX_K search is enqueued by the one call.  Ids are id_base + row (ignored on an index with
 * caller-assigned ids, which are reported). */
int rass_index_search_scored_device(rass_index_t* idx, const float* d_queries, int nq, int k,
                                    const float* d_boost, int transform, int combine, const float* d_min_score,
                                    const float* d_fn, int n_fn, int64_t fn_rows, int64_t fn_stride,
                                    const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                    int64_t id_base, float* d_out_scores, int64_t* d_out_ids);
/* FUNCTION COLUMN BUILDER: OpenSearch's function_score.functions over the int32 attribute columns into a caller-owned DEVICE
 * block d_fn = float[n_fn][stride] (stride a multiple of 32 and >= the index's rows, 1 <= n_fn <= RASS_MAX_DEVICE_BATCH; n_fn
 * = 1: a shared column whose records all name query 0).  `fns` is a HOST array of n_fns records; the records of one query
 * act in LIST order; at most RASS_MAX_SCORE_FNS (16) records per query per call.  With v the row's value in column `col`:
 *   RASS_FN_GAUSS / _EXP / _LINEAR (decay): d = max(0, |v - origin| - offset); gauss exp(d * d * (ln(decay) / (scale * scale))),
 *     exp exp(d * (ln(decay) / scale)), linear max(0, (s - d) / s) with s = scale / (1 - decay).  origin finite, scale > 0,
 *     offset >= 0, 0 < decay < 1.  A row whose value is RASS_ATTR_MISSING gets 1.0 (OpenSearch's rule for decay on a missing field).
 *   RASS_FN_FIELD_VALUE: modifier(factor * v); RASS_FN_MOD_NONE x, _LOG log10(x), _LOG1P log10(1 + x), _LOG2P log10(2 + x),
 *     _LN ln(x), _LN1P ln(1 + x), _LN2P ln(2 + x), _SQUARE x * x, _SQRT sqrt(x), _RECIPROCAL 1 / x.  On a row without the value,
 *     `missing` stands in for v; with `missing` NaN the function does not apply to that row.  A non-positive argument of a
 *     logarithm (a negative one of sqrt) yields -inf / NaN, and the search then EXCLUDES the row — OpenSearch raises instead.
 *   RASS_FN_WEIGHT: the constant 1.0 (a filter function worth only its weight).
 * `filter`: -1, or an index into d_filters = uint32[n_filters][words] (the allow-list bitmap layout, words >= ceil(rows /
 * 32)): the function applies to the rows whose bit is set.  A function applies to a row when its filter allows it and it is
 * not a field_value miss; its value is weight * kind(v) (weight finite).  The applying functions of a query are folded in list order by
 * score_mode — RASS_FN_SCORE_MULTIPLY, _SUM, _AVG (sum(value_i) / sum(weight_i)), _FIRST, _MAX, _MIN (compare and select), the
 * first applying value starting the fold — and the result is capped: value > max_boost ? max_boost : value (+inf: no cap; NaN
 * refused).  A row to which no function applies gets 1.0.
 * ARITHMETIC: all of it in double on the device, each operation rounded on its own, and rounded to fp32 ONCE, at the store; the
 * per-function constants are derived in double on the host.  A cell built from + - * / sqrt and comparisons alone is what an
 * IEEE fp64 restatement gives; a cell through exp or a logarithm is within one fp32 ulp of it.
 * Rows [0, rows) of every column are written, tombstoned rows too; the padding is left alone.  Parameters outside the ranges
 * above, an unknown kind / modifier / score_mode, a record naming a query outside [0, n_fn), a column outside [0,
 * RASS_MAX_ATTRS) or a filter outside [-1, n_filters), too many records for a query, a stride below the rows or words too
 * short: RASS_ERR_INVALID and nothing is written.  Stream-ordered on the engine's stream; the host array may be reused when
 * the call returns. */
#define RASS_MAX_SCORE_FNS 16
#define RASS_FN_GAUSS 0
#define RASS_FN_EXP 1
#define RASS_FN_LINEAR 2
#define RASS_FN_FIELD_VALUE 3
#define RASS_FN_WEIGHT 4
#define RASS_FN_MOD_NONE 0
#define RASS_FN_MOD_LOG 1
#define RASS_FN_MOD_LOG1P 2
#define RASS_FN_MOD_LOG2P 3
#define RASS_FN_MOD_LN 4
#define RASS_FN_MOD_LN1P 5
#define RASS_FN_MOD_LN2P 6
#define RASS_FN_MOD_SQUARE 7
#define RASS_FN_MOD_SQRT 8
#define RASS_FN_MOD_RECIPROCAL 9
#define RASS_FN_SCORE_MULTIPLY 0
#define RASS_FN_SCORE_SUM 1
#define RASS_FN_SCORE_AVG 2
#define RASS_FN_SCORE_FIRST 3
#define RASS_FN_SCORE_MAX 4
#define RASS_FN_SCORE_MIN 5
typedef struct rass_score_fn {
    int32_t query;      /* the column (query) the function belongs to, [0, n_fn) */
    int32_t kind;       /* RASS_FN_* */
    int32_t col;        /* attribute column (ignored by RASS_FN_WEIGHT) */
    int32_t filter;     /* -1, or the bitmap of d_filters that gates the function */
    int32_t modifier;   /* RASS_FN_MOD_* (RASS_FN_FIELD_VALUE only) */
    int32_t reserved;   /* 0 */
    double weight;
    double origin, scale, offset, decay;    /* decay kinds */
    double factor, missing;                 /* RASS_FN_FIELD_VALUE */
} rass_score_fn_t;
int rass_index_fn_from_attr(rass_index_t* idx, const rass_score_fn_t* fns, int64_t n_fns, int n_fn, int score_mode,
                            double max_boost, const uint32_t* d_filters, int n_filters, int64_t words,
                            float* d_fn, int64_t stride);

/* Semantic TERMS AGGREGATION: per-group hit counts above a min_score — OpenSearch's `"aggs": {"x": {"terms": {"field": ...}}}`
 * under a k-NN clause with a min_score, with a `cardinality` and the hit total thrown in.  The group of a row is a bit field
 * of its tag, as in rass_index_search_grouped.  A row is a HIT of query q when it is live, passes q_filter (NULL, exact, or
 * masked by q_filter_mask) and its score is >= min_score[q], as in rass_index_search_range (-inf: every live matching row;
 * NaN: RASS_ERR_INVALID in the host variant, no hits in the device variant).  ONE corpus pass per launch group counts the
 * hits of every (query, group) and keeps each group's best hit; a select over the n_groups counters of each query finishes it.
 * Buckets come in OpenSearch's default order, doc_count descending then group key ascending; the `size` first are listed:
 * out_groups / out_counts / out_scores / out_ids are [nq][size] — the group key, its number of hits, and the score and id of
 * its best hit under (score descending, row ordinal ascending) — and (-1, 0, -inf, -1) past the end.  Scores and ids as
 * rass_index_search_grouped reports them (the flat scan's fp32 scores bit for bit; ordinals or rass_index_add_ex ids).
 * out_n_buckets[q] is the EXACT number of groups with a hit (the field's cardinality among the hits), out_total_hits[q] the
 * EXACT number of hits: what rass_index_search_range reports as its total for the same threshold and filter.  Counts are
 * integers added with atomics: the answer is a function of the index and the arguments alone.
 * group_mask: non-zero, within 0x7fffffff.  n_groups: the exclusive bound of the group key, 1 .. 1 048 576 (the call keeps
 * nq x n_groups 12-byte slots on the device — up to 384 MiB for 32 queries at the bound — in the engine-owned block of the
 * grouped search, grown on demand; RASS_ERR_OOM when it cannot be had, and nothing has changed).
 * 1 <= size <= RASS_MAX_K_MULTIPASS.  Outside those: RASS_ERR_INVALID.  A hit whose group key is >= n_groups is left out of
 * the answer: RASS_ERR_INVALID, named in rass_last_error(), and the outputs are unspecified; a row below the threshold never
 * causes that.  Any nq (scanned in groups of RASS_MAX_QBATCH).  fp32 indices of every dim the engine takes, wide rows
 * included; a bf16 index answers RASS_ERR_UNSUPPORTED.  The prefilter mode of the index is ignored: a candidate scan cannot
 * bound a count.  IVF, cross-index batches, the sharded multi-GPU front and the 64-query pair kernel have no aggregate form;
 * a bitmap restricts rass_index_aggregate_keys.  Thread-safety and layout epochs as rass_index_search_grouped. */
int rass_index_aggregate(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                         int32_t group_mask, int32_t n_groups,
                         const int32_t* q_filter, const int32_t* q_filter_mask,
                         int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                         int64_t* out_n_buckets, int64_t* out_total_hits);
/* Device-resident variant: every pointer is device memory, the call is stream-ordered, nothing is synchronised and nothing is
 * read back; nq <= RASS_MAX_QBATCH.  Ids are id_base + row (ignored on an index with caller-assigned ids, which are
 * reported), to be paired with the layout epoch read before the call.  *d_status = 1 when a hit's group key was >= n_groups
 * (that hit is left out of every figure; the rest of the answer is intact), else 0. */
int rass_index_aggregate_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                int32_t group_mask, int32_t n_groups,
                                const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                int64_t id_base, int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores,
                                int64_t* d_out_ids, int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status);

/* KEY COLUMNS: the group of a row from any attribute column, or from the caller.  A key column is int32[n_keys] in DEVICE
 * memory, owned by the caller as a bitmap is: key g with 0 <= g < n_groups places row r in group g; RASS_KEY_NONE, or any
 * negative key, means the row belongs to NO group — it is neither a match nor a hit and is left out of every figure; a key
 * >= n_groups on a matching row raises the status word exactly as an out-of-range tag key does.  A key column names rows of
 * ONE layout epoch, as a bitmap does.
 * The builders write d_keys[0 .. n_keys), n_keys >= the index's rows at the call (else RASS_ERR_INVALID and d_keys is left
 * untouched); entries [rows, n_keys) are RASS_KEY_NONE.  They are stream-ordered on the engine's stream and do not read the
 * tags: the scan skips tombstones itself.  col outside 0 .. RASS_MAX_ATTRS - 1: RASS_ERR_INVALID; every dtype that takes
 * columns takes the builders.  missing_key >= -1 is the key of a row whose value is RASS_ATTR_MISSING (every row of a column
 * that was never set).
 * _keys_from_attr: key = v - base, computed without overflow; a result outside [0, INT32_MAX] becomes RASS_KEY_NONE.  For a
 *   keyword column base = 0, missing_key = 0 reproduces the tag convention (codes from 1, 0 = none).
 * _keys_from_attr_edges: `edges` is a HOST array (reusable on return: the call synchronises), strictly ascending,
 *   2 <= n_edges <= RASS_MAX_KEY_EDGES, else RASS_ERR_INVALID; key j means edges[j] <= v < edges[j + 1]; a value below the
 *   first edge or at or above the last becomes RASS_KEY_NONE.  A histogram's buckets, a calendar's months.
 * _keys_from_tag: key = (tag & mask) >> ctz(mask) of a live row, RASS_KEY_NONE for a tombstone: the group of the tag-keyed
 *   calls as a key column, so that they can run within a bitmap.  mask: non-zero, within 0x7fffffff.
 * _attr_minmax: min, max and count of the present values of column col over the LIVE rows, by one small reduction; it
 *   synchronises.  *out_n_present == 0 (a column never set, an empty index) leaves *out_min / *out_max unspecified. */
int rass_index_keys_from_attr(rass_index_t* idx, int col, int32_t base, int32_t missing_key, int32_t* d_keys, int64_t n_keys);
int rass_index_keys_from_attr_edges(rass_index_t* idx, int col, const int32_t* edges, int n_edges, int32_t missing_key,
                                    int32_t* d_keys, int64_t n_keys);
int rass_index_keys_from_tag(rass_index_t* idx, int32_t mask, int32_t* d_keys, int64_t n_keys);
int rass_index_attr_minmax(rass_index_t* idx, int col, int32_t* out_min, int32_t* out_max, int64_t* out_n_present);
/* rass_index_search_grouped and rass_index_aggregate with the group of a row taken from a key column, optionally within a
 * row bitmap: "the best chunk per source document", "hits per condition code", "hits per month under a date range".  The tag
 * is still read for tombstones and for q_filter / q_filter_mask.  d_keys and d_allow are DEVICE memory in the host variants
 * too: a key column is 4 bytes per row and is built where it is used; the caller orders its own writes to them before the
 * call.  n_keys >= the index's rows at the call, else RASS_ERR_INVALID.  d_allow may be NULL (no restriction); otherwise it is
 * uint32[n_bitmaps][words_per_bitmap] as rass_index_search_allowed takes it, n_bitmaps 1 (shared) or nq, words_per_bitmap >=
 * ceil(rows / 32), else RASS_ERR_INVALID; a row then also needs its bit.  A bitmap on a wide-row index (dim > 1024) answers
 * RASS_ERR_UNSUPPORTED; keys alone run on every dim.  With a bitmap the scan still streams EVERY tile of the slab — only the
 * emission is restricted; a plan-driven walk over the tiles with a bit set, as the allow-list search has, is not built.
 * Everything else — the bounds on k / size and n_groups, padding values, result order, the status word and RASS_ERR_INVALID
 * for a key >= n_groups, the engine-owned table block, fp32 indices only, one layout per answer — is exactly that of the
 * tag-keyed calls, and scores are the flat scan's, bit for bit.  out_group_total and out_total_hits / out_n_buckets count
 * only rows that have a group. */
int rass_index_search_grouped_keys(rass_index_t* idx, const float* queries, int nq, int k,
                                   const int32_t* d_keys, int64_t n_keys, int32_t n_groups,
                                   const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                   const int32_t* q_filter, const int32_t* q_filter_mask,
                                   float* out_scores, int64_t* out_ids, int32_t* out_groups,
                                   int64_t* out_group_total);
int rass_index_search_grouped_keys_device(rass_index_t* idx, const float* d_queries, int nq, int k,
                                          const int32_t* d_keys, int64_t n_keys, int32_t n_groups,
                                          const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                          const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                          int64_t id_base, float* d_out_scores, int64_t* d_out_ids,
                                          int32_t* d_out_groups, int64_t* d_group_total, int32_t* d_status);
/* INNER HITS of the grouped search over a key column: the group_size best rows of each of a query's k best groups — OpenSearch's
 * collapse + inner_hits {size: n}, or terms -> top_hits — and, optionally, the CAPPED list: the exact top-k of all live matching
 * rows with at most group_size rows taken from any one group ("the best k chunks, at most m per source document").  One corpus
 * pass per launch group, whatever group_size is.  Arguments as rass_index_search_grouped_keys(_device), plus:
 * group_size in [1, RASS_MAX_GROUP_SIZE], with n_groups * group_size <= 1048576 (the engine-owned table of a 32-query launch
 *   group then stays within the grouped search's 256 MiB; it is grown on demand, and RASS_ERR_OOM leaves the engine as it was);
 * out_scores / out_ids [nq][k][group_size]: group j of query q (the grouped search's j-th: out_groups [nq][k] and
 *   out_group_total [nq] are exactly what rass_index_search_grouped_keys reports) holds its rows best first under (score
 *   descending, row ascending); entry [q][j][0] is the grouped search's [q][j]; (-inf, -1) past a group's last matching row and
 *   for a missing group;
 * out_capped_scores / out_capped_ids [nq][k], both or neither (NULL: skipped): the capped list, best first under (score
 *   descending, row ordinal ascending) whatever ids the rows carry, (-inf, -1) past the end.  It needs k * group_size <=
 *   RASS_MAX_K_MULTIPASS.  With group_size >= the largest group it is the plain top-k.
 * k <= RASS_MAX_K_MULTIPASS; any bound broken: RASS_ERR_INVALID.  fp32 flat indices with dim <= 1024 only: a bf16 index or a
 * wide-row index answers RASS_ERR_UNSUPPORTED.  The prefilter mode is ignored: always the exact fp32 scan, and a score is the
 * flat scan's bit for bit.  The host variant takes any nq in launch groups of 32 and fails with RASS_ERR_INVALID where a
 * matching row's key is >= n_groups; the device variant takes nq <= RASS_MAX_DEVICE_BATCH in launch groups of 32, is
 * stream-ordered, synchronises nothing and reports that condition as *d_status = 1 (0 otherwise). */
#define RASS_MAX_GROUP_SIZE 16
int rass_index_search_group_hits_keys(rass_index_t* idx, const float* queries, int nq, int k,
                                      const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int group_size,
                                      const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                      const int32_t* q_filter, const int32_t* q_filter_mask,
                                      float* out_scores, int64_t* out_ids, int32_t* out_groups,
                                      int64_t* out_group_total, float* out_capped_scores, int64_t* out_capped_ids);
int rass_index_search_group_hits_keys_device(rass_index_t* idx, const float* d_queries, int nq, int k,
                                             const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int group_size,
                                             const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                             const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                             int64_t id_base, float* d_out_scores, int64_t* d_out_ids,
                                             int32_t* d_out_groups, int64_t* d_group_total,
                                             float* d_out_capped_scores, int64_t* d_out_capped_ids, int32_t* d_status);
int rass_index_aggregate_keys(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                              const int32_t* d_keys, int64_t n_keys, int32_t n_groups,
                              const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                              const int32_t* q_filter, const int32_t* q_filter_mask,
                              int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                              int64_t* out_n_buckets, int64_t* out_total_hits);
int rass_index_aggregate_keys_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                     const int32_t* d_keys, int64_t n_keys, int32_t n_groups,
                                     const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                     const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                     int64_t id_base, int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores,
                                     int64_t* d_out_ids, int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status);
/* STATS SUB-AGGREGATION: rass_index_aggregate_keys(_device) with the count, sum, min and max of an attribute column over each
 * bucket's hits — OpenSearch's `stats` / `min` / `max` / `sum` / `avg` / `value_count` metrics under a `terms` or `histogram`
 * aggregation, `"order": {"<metric>": "asc" | "desc"}`, or, with d_keys NULL, on their own.  Still ONE corpus pass per launch
 * group: the scan keeps, per (query, group), the hit count, the best hit, and the count / sum / min / max of the hits' values
 * in column value_col; then one select over the query's groups and one gather of the listed buckets.  All of it is integer
 * arithmetic on int32 values: the answer is a function of the index and the arguments alone.  Arguments, hit test, padding,
 * totals, ids, status word, filters, bitmap, tombstones, layout epochs and locking as rass_index_aggregate_keys(_device), plus:
 * d_keys NULL with n_groups == 1: the GLOBAL form — every row is in group 0, n_keys is not read.  NULL with any other
 *   n_groups: RASS_ERR_INVALID.
 * value_col in [0, RASS_MAX_ATTRS), else RASS_ERR_INVALID.  A hit whose value is RASS_ATTR_MISSING (every row of a column
 *   that was never set) counts in out_counts and not in the metrics.
 * order_by, order_desc (0: ascending, else descending): the bucket order before the `size` first are listed.
 *   RASS_STATS_BY_COUNT descending is rass_index_aggregate_keys' order, and groups / counts / scores / ids / n_buckets /
 *   total_hits are then exactly what that call reports.  _BY_VALUE_COUNT, _BY_MIN, _BY_MAX order by that metric.  Only buckets
 *   with a hit are listed; ties break by group key ascending; a bucket with no present value comes after every bucket that
 *   has one, in BOTH directions, by group key ascending.  Any other order_by: RASS_ERR_INVALID.  (Ordering by sum or avg has
 *   no device form: a caller that lists every bucket orders them itself.)
 * out_value_counts / out_sums (int64) and out_mins / out_maxs (int32), each [nq][size]: per listed bucket the number of hits
 *   with a value, their exact sum, the smallest and the largest; (0, 0, 0, 0) for a bucket with no present value and past the
 *   last bucket.  avg = sum / value_count is the caller's division.
 * The table is nq x n_groups 32-byte slots in the engine-owned block of the grouped search — 1 GiB for 32 queries at the
 *   n_groups bound — grown on demand; RASS_ERR_OOM leaves the engine as it was.
 * A bound broken, or a NaN min_score in the host variant: RASS_ERR_INVALID, nothing is launched and the outputs are untouched.
 * fp32 flat indices with dim <= 1024 only: a bf16 index or a wide-row index answers RASS_ERR_UNSUPPORTED.  The prefilter mode
 * is ignored: always the exact fp32 scan, and a score is the flat scan's bit for bit.  The host variant takes any nq in launch
 * groups of RASS_MAX_QBATCH and fails with RASS_ERR_INVALID where a hit's key is >= n_groups; the device variant takes nq <=
 * RASS_MAX_QBATCH, is stream-ordered, synchronises nothing and reports that condition as *d_status = 1 (0 otherwise). */
#define RASS_STATS_BY_COUNT 0
#define RASS_STATS_BY_VALUE_COUNT 1
#define RASS_STATS_BY_MIN 2
#define RASS_STATS_BY_MAX 3
int rass_index_aggregate_stats_keys(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                                    const int32_t* d_keys, int64_t n_keys, int32_t n_groups,
                                    int value_col, int order_by, int order_desc,
                                    const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                    const int32_t* q_filter, const int32_t* q_filter_mask,
                                    int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                                    int64_t* out_value_counts, int64_t* out_sums, int32_t* out_mins, int32_t* out_maxs,
                                    int64_t* out_n_buckets, int64_t* out_total_hits);
int rass_index_aggregate_stats_keys_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                           const int32_t* d_keys, int64_t n_keys, int32_t n_groups,
                                           int value_col, int order_by, int order_desc,
                                           const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                           const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                           int64_t id_base, int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores,
                                           int64_t* d_out_ids, int64_t* d_out_value_counts, int64_t* d_out_sums,
                                           int32_t* d_out_mins, int32_t* d_out_maxs, int64_t* d_n_buckets,
                                           int64_t* d_total_hits, int32_t* d_status);
/* TOP HITS SUB-AGGREGATION: rass_index_aggregate_keys(_device) with the top_hits best hits of every listed bucket — OpenSearch's
 * `terms` -> `top_hits {size: n}`, the buckets ordered by doc_count or by `"order": {"max_score": "desc"}`.  Still ONE corpus
 * pass per launch group, whatever top_hits is: the scan keeps, per (query, group), the hit count and a chain of top_hits slots
 * that ends as the group's best hits (as rass_index_search_group_hits_keys keeps its rows, here for the hits above min_score
 * only); then one select over the query's groups and one finish over the listed buckets.  Arguments, hit test, totals, ids
 * (id_base, caller-assigned ids), status word, filters, bitmap, tombstones, RASS_KEY_NONE, n_keys >= rows, layout epochs and
 * locking as rass_index_aggregate_keys(_device), plus:
 * top_hits in [1, RASS_MAX_GROUP_SIZE], with n_groups * top_hits <= 1048576 (the engine-owned table, grown on demand;
 *   RASS_ERR_OOM leaves the engine as it was).
 * order_by: RASS_AGG_BY_COUNT — doc_count descending, then key ascending: rass_index_aggregate_keys' order, and groups /
 *   counts / n_buckets / total_hits are exactly what that call reports; RASS_AGG_BY_SCORE — by each bucket's best hit under
 *   (score descending, row ordinal ascending).  Only buckets with a hit are listed either way.  Any other: RASS_ERR_INVALID.
 * out_groups / out_counts [nq][size]; out_scores / out_ids [nq][size][top_hits]: bucket j's hits best first under (score
 *   descending, row ordinal ascending); entry [q][j][0] is what rass_index_aggregate_keys reports as the bucket's best hit.
 *   (-inf, -1) past a bucket's last hit; (-1, 0, -inf, -1) past the last bucket.
 * 1 <= size <= RASS_MAX_K_MULTIPASS.  A bound broken, or a NaN min_score in the host variant (on the device it matches
 * nothing): RASS_ERR_INVALID, nothing is launched and the outputs are untouched.  fp32 flat indices with dim <= 1024 only: a
 * bf16 index or a wide-row index answers RASS_ERR_UNSUPPORTED.  The prefilter mode is ignored: always the exact fp32 scan, and
 * a score is the flat scan's bit for bit.  The host variant takes any nq in launch groups of RASS_MAX_QBATCH and fails with
 * RASS_ERR_INVALID where a hit's key is >= n_groups; the device variant takes nq <= RASS_MAX_QBATCH, is stream-ordered,
 * synchronises nothing and reports that condition as *d_status = 1 (0 otherwise). */
#define RASS_AGG_BY_COUNT 0
#define RASS_AGG_BY_SCORE 1
int rass_index_aggregate_hits_keys(rass_index_t* idx, const float* queries, int nq, const float* min_score, int size,
                                   const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int top_hits, int order_by,
                                   const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                   const int32_t* q_filter, const int32_t* q_filter_mask,
                                   int32_t* out_groups, int64_t* out_counts, float* out_scores, int64_t* out_ids,
                                   int64_t* out_n_buckets, int64_t* out_total_hits);
int rass_index_aggregate_hits_keys_device(rass_index_t* idx, const float* d_queries, int nq, const float* d_min_score, int size,
                                          const int32_t* d_keys, int64_t n_keys, int32_t n_groups, int top_hits, int order_by,
                                          const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                          const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                          int64_t id_base, int32_t* d_out_groups, int64_t* d_out_counts, float* d_out_scores,
                                          int64_t* d_out_ids, int64_t* d_n_buckets, int64_t* d_total_hits, int32_t* d_status);

/* GRAM matrices of short row lists: out[l][i][j] = the fp32 dot product of stored rows rows[l][i] and rows[l][j], as they lie
 * in the slab (normalised at add time: their cosine).  The similarity structure of a result set, duplicate detection over an
 * appended batch, and the candidate x candidate input of rass_index_search_mmr.
 * rows is [n_lists][list_len] row ORDINALS of one layout of the index, 1 <= list_len <= RASS_MAX_MMR_FETCH, n_lists >= 1
 * (staged in groups; no upper bound); out is [n_lists][list_len][list_len].  PADDING is an ordinal < 0 or >= the row count,
 * or a tombstoned row: +0.0 in its whole row and column.  An ordinal may repeat.
 * Every element is ONE v_mfma_f32_16x16x4_f32 chain over the columns (a k-ordered fp32 fma chain from zero, in the kernel's
 * own column order), the same whatever n_lists, list_len and the position in the list are, and the same inside
 * rass_index_search_mmr: equal bits everywhere.  out is bitwise symmetric.  The rows are read straight out of the slab (the
 * gather is fused into the MFMA operand loads): no workspace beyond the 2 MiB staging of the host variant.
 * fp32 indices of every dim the engine takes, wide rows included; a bf16 index answers RASS_ERR_UNSUPPORTED.  Synchronises. */
int rass_index_rows_gram(rass_index_t* idx, const int64_t* rows, int n_lists, int list_len, float* out);
/* Device-resident variant: d_rows and d_out are device memory, the call is stream-ordered on the engine's stream, nothing is
 * synchronised and nothing is read back. */
int rass_index_rows_gram_device(rass_index_t* idx, const int64_t* d_rows, int n_lists, int list_len, float* d_out);

/* DIVERSIFIED (MMR) search: a greedy maximal-marginal-relevance re-rank of the exact top fetch_k — what a RAG caller asks for
 * when near-identical chunks would otherwise fill the prompt.  For query q, with 1 <= k <= fetch_k <= RASS_MAX_MMR_FETCH and
 * lambda[q] in [0, 1]:
 * CANDIDATES: the list rass_index_search_ex(k = fetch_k) returns for q on the exact fp32 scan — the same filter semantics
 * (q_filter NULL, exact, or (tag & q_filter_mask[q]) == q_filter[q]), live rows only, score descending, id ascending.
 * Candidate i (its RANK) has score s_i, bit-identical to what rass_index_search_ex reports; c <= fetch_k is the number of
 * real candidates.  The prefilter mode of the index is ignored, as in the range and grouped searches: always the exact scan.
 * SIMILARITY: G[i][j] = what rass_index_rows_gram reports for the candidates' rows (bit for bit: the same kernel).
 * SELECTION, all in fp32, every operation rounded on its own (no fused multiply-add): l = lambda[q], m = 1 - l; pen_i is
 * undefined while nothing is selected.  At each of min(k, c) steps, for every unselected i < c:
 *     obj_i = (l * s_i) - (m * pen_i)          the second product taken as +0.0 at the first step
 * the largest obj_i is picked, ties to the lowest rank i.  After picking p: pen_i = G[p][i] if it was undefined, else
 * G[p][i] where G[p][i] > pen_i, else pen_i (the maximum; negative similarities are NOT clipped to zero).
 * OUTPUT, in selection order: out_scores[q][t] = s_p (the raw cosine to the query, not the objective), out_ids[q][t] = p's id
 * as rass_index_search_ex reports it, out_rank[q][t] = p (int32; out_rank may be NULL); (-inf, -1, -1) past min(k, c).
 * lambda = 1 reproduces rass_index_search_ex(k) bit for bit; lambda = 0 picks the best hit, then always the candidate least
 * similar to everything picked so far.
 * Host pointers, any nq (in groups of RASS_MAX_QBATCH); lambda is nq floats.  A NaN or out-of-range lambda, k > fetch_k or
 * fetch_k > RASS_MAX_MMR_FETCH: RASS_ERR_INVALID.  Cost: ceil(fetch_k / 32) corpus passes per group (chained on the device by
 * the continuation bound), then one Gram launch and one selection launch.
 * fp32 indices of every dim the engine takes, wide rows included; a bf16 index answers RASS_ERR_UNSUPPORTED.  An index with
 * caller-assigned ids (rass_index_add_ex) is served with the limit rass_index_search_ex has: fetch_k <= RASS_MAX_K, beyond:
 * RASS_ERR_UNSUPPORTED.  IVF, cross-index batches and the sharded multi-GPU front have no MMR form.
 * Thread-safety and layout epochs as rass_index_search_ex: the engine lock is held while enqueuing only, and the answer
 * comes from ONE layout of the index. */
int rass_index_search_mmr(rass_index_t* idx, const float* queries, int nq, int k, int fetch_k,
                          const float* lambda, const int32_t* q_filter, const int32_t* q_filter_mask,
                          float* out_scores, int64_t* out_ids, int32_t* out_rank);
/* Device-resident variant: every pointer is device memory, the call is stream-ordered, nothing is synchronised and nothing is
 * read back; nq <= RASS_MAX_QBATCH.  Every pass of the candidate search is enqueued by the one call.  Ids are id_base + row
 * (ignored on an index with caller-assigned ids, which are reported), to be paired with the layout epoch read before the
 * call.  A query whose lambda is NaN or outside [0, 1] gets the EMPTY list (every slot (-inf, -1, -1)): it cannot be refused
 * without reading it back.  d_out_rank may be NULL. */
int rass_index_search_mmr_device(rass_index_t* idx, const float* d_queries, int nq, int k, int fetch_k,
                                 const float* d_lambda, const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                 int64_t id_base, float* d_out_scores, int64_t* d_out_ids, int32_t* d_out_rank);

/* Prefilter mode (SURVEY §8f-4 "bf16 (or int8)"; the reference's own index is approximate, app/main.py:563-572), OFF by
 * default.  `enable` = RASS_PREFILTER_BF16 (1): keep a bf16 copy of the slab, scan IT (half the HBM bytes per pass, bf16
 * MFMA) for the 32 best candidates per query; RASS_PREFILTER_INT8 (2): keep an int8 copy (a quarter of the bytes; per row
 * q = rint(x * 127 / max|x|) and one fp32 scale, queries quantised the same way, v_mfma_i32_16x16x64_i8; a candidate's score
 * is (float)(exact integer dot) * row scale).  Either way those candidates' scores are then recomputed exactly from the fp32
 * slab in the flat kernel's fmaf order and the exact top-k among them is returned: returned scores are bit-identical to the
 * flat path; the id set equals the flat result whenever the true top-k lies inside the candidate top-32 (measured as recall,
 * not guaranteed).  Used for k <= 16 only (k > 16 takes the exact flat scan).  bf16 needs dim padded to a multiple of 256 and
 * dim <= 1024; int8 serves every dim an index takes (wide rows, 1024 < dim <= 2048, included).  0 = off (frees the copy);
 * switching modes rebuilds the copy from the fp32 rows. */
#define RASS_PREFILTER_OFF 0
#define RASS_PREFILTER_BF16 1
#define RASS_PREFILTER_INT8 2
/* RASS_PREFILTER_INT8_EXACT (3): certified int8 search — answers are the flat scan's, ids and scores, bit for bit, for every
 * query with k <= 32.  Per pass of 16 queries: an int8 scan with each query carried as hi + lo int8 vectors keeps the 128 best
 * candidates, they are re-ranked exactly in fp32, a per-query certificate (DESIGN.md §3 "certified int8 search") proves that no
 * row outside them can enter the top-k, and the exact fp32 flat scan runs for the queries whose certificate fails.  Every
 * device search API stays stream-ordered (the fallback reads its query count on the device).  k > 32 takes the exact passes. */
#define RASS_PREFILTER_INT8_EXACT 3
int rass_index_set_prefilter(rass_index_t* idx, int enable);
int rass_index_get_prefilter(const rass_index_t* idx);   /* the mode: 0 / 1 / 2 / 3 */
/* Mode 3's device counters since the mode was set (searched queries, certified queries, queries that took the fp32
 * fallback) and the certificate's row maxima R = max |y - s_y y8|, V = max |s_y y8|.  Synchronises the engine's stream. */
int rass_index_certify_stats(rass_index_t* idx, int64_t* queries, int64_t* certified, int64_t* fallbacks, float* R, float* V);
/* Mode 3's parity hook for <= 32 device queries: the 128 candidates per query the certificate covers ([nq][128] int8
 * candidate scores and LOCAL rows, (score desc, row asc), -inf / -1 past the end), tau [nq] (every eligible row outside the
 * list scores at most tau; -inf: none is outside) and the certificate flags [nq] (1 = certified at this k).  Stream-ordered.
 * RASS_ERR_UNSUPPORTED unless the index is in mode 3. */
int rass_index_candidates_exact_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                       float* d_cand_scores, int64_t* d_cand_rows, float* d_tau, int32_t* d_certified);
/* The sample floor's parity hook for a fused fp32 batch (nq > 32 device queries on an fp32 index without prefilter): the
 * normalise launch and the sample stage exactly as rass_index_search_device_batch would run them for this nq and k, then, per
 * query, the 32 representative rows ([nq][32] LOCAL rows, one per block of the slab's sample prefix; -1: the block has no row
 * the query may rank) and their scores ([nq][32], the flat scan's score of that row bit for bit; -inf: no representative, or a
 * score that is not finite).  The floor of a query is the k-th largest of its 32 scores.  Stream-ordered.
 * RASS_ERR_UNSUPPORTED where the batch would not take that stage (small slab, ragged nq, RASS_SCAN_BATCH_SAMPLE=f32 / groups,
 * RASS_SCAN_SAMPLE_FLOOR=0). */
int rass_index_sample_floor_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                   int32_t* d_out_rows, float* d_out_scores);
/* Beside it: the ONE floor per query that the batch computes from those 32 scores, once per call, for its step-kernel launches
 * ([nq] floats): the largest value of the top 20 bits of the scores' order-preserving keys that at least k of the query's 32
 * scores reach — at most the k-th largest of them, below it by < 2^-11 of its value — and -inf where fewer than k of them are
 * above -inf.  Same conditions, same RASS_ERR_UNSUPPORTED. */
int rass_index_step_floors_device(rass_index_t* idx, const float* d_queries, int nq, int k, const int32_t* d_q_filter,
                                  float* d_out_floors);
/* The candidate lists of the active prefilter mode for <= 32 device queries, BEFORE the exact re-rank: [nq][32] candidate
 * scores (bf16: fp32-accumulated dot of the bf16-rounded operands; int8: as above) and LOCAL rows, (score desc, row asc),
 * -inf / -1 past the end.  Parity hook of the integer path (tests compare it with the oracle bit for bit); stream-ordered.
 * RASS_ERR_UNSUPPORTED in mode 3 (rass_index_candidates_exact_device). */
int rass_index_candidates_device(rass_index_t* idx, const float* d_queries, int nq, const int32_t* d_q_filter,
                                 float* d_cand_scores, int64_t* d_cand_rows);

/* Shard persistence: raw rows + tags + manifest header. */
int rass_index_save(rass_index_t* idx, const char* path);
int rass_index_load(rass_engine_t* eng, const char* name, const char* path,
                    rass_index_t** out);

/* Fill rows [first, first+n) of the index with synthetic unit vectors
 * generated ON DEVICE (counter-based RNG keyed by (seed, global row id), so
 * any shard regenerates identically; SURVEY §8d cfg 2/4).  Appends when
 * first == rass_index_rows().  `row_id_base` offsets the RNG key for sharding. */
int rass_index_fill_synthetic(rass_index_t* idx, int64_t n, uint64_t seed,
                              int64_t row_id_base);

/* --------------------------------------------- stateless kernel launchers */

/* Bytes of scratch the scan needs for (nq, k). */
size_t rass_scan_workspace_bytes(int nq, int k);

/* Corpus layout in HBM ("tile16"): rows live in 16-row blocks of 16*row_stride
 * floats; inside a block, chunk j (columns 16j..16j+15) of the 16 rows is one
 * contiguous 1 KiB in MFMA lane order, i.e. element (row r, col c) sits at
 *   (r>>4)*16*row_stride + (c>>4)*256 + ((((c>>2)&3)*16 + (r&15))*4) + (c&3)
 * floats from the slab base.  Every wave-level load of the scan is then a fully
 * coalesced 1 KiB burst that already is the MFMA A operand.  row_stride = dim
 * rounded up to 128 (to 256 above 1024 columns), zero padded; a slab holds
 * whole blocks (rows rounded up to 16).  The two converters below move between
 * row-major and tile16. */
int rass_pack_rows_f32(const float* d_in, int64_t in_stride, float* d_packed,
                       int64_t row_stride, int64_t first_row, int64_t n, int dim,
                       int normalize, void* stream);
int rass_unpack_rows_f32(const float* d_packed, int64_t row_stride,
                         int64_t first_row, int64_t n, int dim, float* d_out,
                         int64_t out_stride, void* stream);
/* d_out[i] (row-major, out_stride) <- row d_row_ids[i] of a tile16 slab holding n_rows rows, i < n (device arrays): the
 * scattered form of rass_unpack_rows_f32 (k-means seeds are nlist sample rows all over the slab). */
int rass_gather_rows_f32(const float* d_packed, int64_t row_stride, int64_t n_rows,
                         const int64_t* d_row_ids, int64_t n, int dim, float* d_out,
                         int64_t out_stride, void* stream);
/* The two steps of rass_index_compact on caller-owned arrays (all device, stream-ordered, stateless).
 * rass_compact_plan: d_tags[n_rows] -> d_new_row[n_rows] (the number of live rows below r, -1 where
 *   d_tags[r] == RASS_ROW_TAG_DELETED), d_src_row[j] = the old row that becomes row j (j < n_live; give it
 *   n_rows entries) and *d_n_live.  Three launches; no workgroup waits on another.  d_workspace: at least
 *   rass_compact_plan_workspace_bytes(n_rows) bytes.
 * rass_compact_rows_f32: tile16 slab d_dst (whole blocks, >= round_up(n_dst, 16) rows) <- rows
 *   d_src_row[0 .. n_dst) of the tile16 slab d_src (n_src_rows rows; an entry outside it gives a zero row);
 *   the rows of the last block past n_dst are zeroed.  Rows are moved, bit for bit.  d_dst != d_src. */
int rass_compact_plan(const int32_t* d_tags, int64_t n_rows, int64_t* d_new_row,
                      int64_t* d_src_row, int64_t* d_n_live, void* d_workspace,
                      size_t workspace_bytes, void* stream);
size_t rass_compact_plan_workspace_bytes(int64_t n_rows);
int rass_compact_rows_f32(const float* d_src, float* d_dst, int64_t row_stride,
                          const int64_t* d_src_row, int64_t n_dst, int64_t n_src_rows,
                          void* stream);

/* K1+K2: fused flat cosine scan + per-workgroup top-k + merge over a tile16
 * fp32 corpus slab in HBM.  Rows must already be normalised (rass_pack_rows_f32
 * with normalize=1 does both); d_queries (nq x dim, row-major) are normalised
 * by the launcher.  row_stride is in elements, 128 * {1..8} or (wide rows)
 * 256 * {5..8}, with zero padding beyond dim; the slab must hold
 * ceil(n_rows/16) whole blocks.
 * d_row_tag / d_q_filter may be NULL. */
int rass_scan_topk_f32(const float* d_corpus, int64_t n_rows, int dim,
                       int64_t row_stride, const int32_t* d_row_tag,
                       const float* d_queries, int nq,
                       const int32_t* d_q_filter, int k, int64_t id_base,
                       float* d_out_scores, int64_t* d_out_ids,
                       void* d_workspace, size_t workspace_bytes,
                       void* stream);

/* K2/K3 merge: n_lists sorted candidate lists per query, laid out
 * [n_lists][nq][k] (score f32, id i64; id < 0 = empty), -> [nq][k] with the
 * same total order.  Used after the RCCL all-gather of per-shard top-k. */
int rass_topk_merge(const float* d_scores, const int64_t* d_ids, int n_lists,
                    int nq, int k, float* d_out_scores, int64_t* d_out_ids,
                    void* stream);

/* Same with explicit list strides (in elements): lets the merge read the G
 * per-rank records of ONE all-gather, each packed as nq*k f32 scores followed
 * by nq*k i64 ids, without unpacking (rassengine_amd/dist.py). */
int rass_topk_merge_strided(const float* d_scores, const int64_t* d_ids,
                            int64_t score_list_stride, int64_t id_list_stride,
                            int n_lists, int nq, int k, float* d_out_scores,
                            int64_t* d_out_ids, void* stream);

/* The same merge for several launch groups in ONE launch: query q of nq_total belongs to group q / group_size,
 * whose lists start g * score_group_stride / id_group_stride elements after group 0's (the gathered
 * [rank][group][record] buffer of dist.ShardedSearch.search_batch); output contiguous [nq_total][k]. */
int rass_topk_merge_strided_batch(const float* d_scores, const int64_t* d_ids,
                                  int64_t score_list_stride, int64_t id_list_stride,
                                  int n_lists, int nq_total, int group_size,
                                  int64_t score_group_stride, int64_t id_group_stride, int k,
                                  float* d_out_scores, int64_t* d_out_ids, void* stream);

/* the cross-shard exchange without a collective.  Rank 0 creates a buffer in its HBM and hands
 * the 64-byte HIP IPC handle to the other ranks' processes (one process per GPU); every rank then STORES its
 * packed per-shard top-k record into its slot (over xGMI between GPUs) and releases a per-rank sequence flag at
 * system scope (rass_peer_post: copy, fence, flag); rank 0 enqueues rass_peer_wait (one workgroup acquiring the
 * n flags, BOUNDED: after max_spins polls it gives up and stores 1 + the missing rank in *d_status instead of
 * hanging the GPU) in front of its rass_topk_merge_strided.  Replaces the OpenSearch shard -> coordinator
 * response (SHARD_COUNT, app/main.py:89, 357).  Layout and step protocol: rassengine_amd/dist.py
 * (PeerMergeSearch).  The processes need HSA_ENABLE_IPC_MODE_LEGACY=0 on this platform. */
int rass_peer_buffer_create(int device, size_t bytes, void** d_ptr, unsigned char* handle64);
int rass_peer_buffer_open(int device, const unsigned char* handle64, void** d_ptr);
int rass_peer_buffer_close(void* d_ptr, int opened_from_handle);
int rass_peer_post(const void* d_record, size_t bytes, void* d_remote_slot, void* d_remote_flag,
                   uint64_t seq, void* stream);
int rass_peer_wait(const void* d_flags, int n, int flag_stride_bytes, uint64_t seq, int* d_status,
                   int64_t max_spins, void* stream);

/* a4 (app/main.py:1249-1251, 1536-1537): out = in / (||in||_2 + 1e-9), rows
 * of `dim` floats read at in_stride, written at out_stride (elements); the
 * out_stride - dim tail of each output row is zero-filled. */
int rass_normalize_rows_f32(const float* d_in, int64_t in_stride, float* d_out,
                            int64_t out_stride, int64_t n, int dim,
                            void* stream);

/* -------------------------------------------------------------------- IVF
 * K9: inverted-file cosine index (nlist coarse centroids + contiguous lists)
 * for shards where a flat scan per query batch is too much (BASELINE cfg 5:
 * 100 M rows, IVF-4096).  Stands in for the sub-linear behaviour of the
 * reference's HNSW (app/main.py:563-572) while staying an HBM-streaming
 * kernel: probing = the flat fused scan over the centroid slab, a plan kernel,
 * and the same fused scan over the union of the batch's probed lists.
 * Approximate by construction: recall@k vs the flat index is a function of
 * nprobe and is measured, never assumed (nprobe = nlist is exact). */
typedef struct rass_ivf rass_ivf_t;

/* K9(i): the two O(rows) steps of spherical k-means, over rows already resident in `idx`'s slab, asynchronous
 * on the engine stream.  The processed rows are 32-row blocks first_block, first_block + block_step, ...
 * (n_blocks of them: a strided training sample, or every block with block_step = 1).
 *   rass_kmeans_assign: d_assign[b*32 + r] = arg max over the nlist centroids of the cosine with row r of the
 *     b-th processed block (exact fp32 MFMA, ties -> lowest list); d_best (may be NULL) the winning cosine.
 *     `d_centroids_tile16`: nlist normalised centroids as a tile16 slab (rass_pack_rows_f32, normalize = 1),
 *     row_stride = rass_index_row_stride(idx), whole 16-row blocks.  Entries of rows past rass_index_rows() or
 *     tombstoned are computed like any other and must be ignored by the caller.
 *   rass_kmeans_accumulate: d_sums[list][0..dim) += row, d_counts[list] += 1 for every processed row below
 *     rass_index_rows() (fp32 atomics; d_sums is nlist x dim row-major, caller-zeroed).
 * The all-reduce over ranks, the normalisation of the sums and the re-seeding of empty lists are O(nlist x dim)
 * and stay with the caller (rassengine_amd/ivf.py).  That caller's training leaves tombstoned rows out: it sets their
 * entries of d_assign to -1 before rass_kmeans_accumulate (which skips a list outside [0, nlist)) and draws no seed,
 * re-seed or repair row among them.  The two primitives themselves do not look at the tags. */
int rass_kmeans_assign(rass_index_t* idx, int64_t first_block, int64_t block_step,
                       int64_t n_blocks, const float* d_centroids_tile16, int nlist,
                       int32_t* d_assign, float* d_best);
int rass_kmeans_accumulate(rass_index_t* idx, int64_t first_block, int64_t block_step,
                           int64_t n_blocks, const int32_t* d_assign, float* d_sums,
                           float* d_counts, int nlist);

/* Build from a flat index: `centroids` nlist x dim fp32 (host; normalised
 * here), `assign[r]` = list of source row r (host, one per appended row;
 * tombstoned rows are skipped).  Training / assignment are offline and live in
 * the Python layer (rassengine_amd/ivf.py).  Result ids are the source index's
 * row ids.  The source index may be dropped afterwards. */
int rass_ivf_build(rass_index_t* src, const float* centroids, int nlist,
                   const int32_t* assign, rass_ivf_t** out);
/* The same with the IVF's list-ordered copy of the rows held as `slab_dtype`: RASS_F32 = rass_ivf_build;
 * RASS_BF16 = the rows rounded to bf16 (half the HBM bytes per probed row; needs the row stride to be a multiple of
 * 256): the fine scan is then the bf16 scan (queries rounded to bf16, fp32 accumulation) and a probe returns what a
 * flat RASS_BF16 index over the same rows returns, restricted to the probed lists.  The source index is fp32 either
 * way (k-means and the assignment read it) and may be dropped afterwards.  (SURVEY §8f-4's bf16 path for cfg 5.)
 * RASS_I8 = an fp32 slab (lists on 64-row tiles) PLUS its int8 copy (per-row-scaled, as rass_index_set_prefilter mode 2): the
 * fine scan reads the int8 copy (a quarter of the bytes per probed row) and keeps 32 candidates per query, which are then
 * rescored exactly from the fp32 slab — returned scores are the fp32 IVF's bit for bit, the id set equals it whenever the
 * probed lists' true top-k lies inside the int8 top-32 (measured as recall).  Serves k <= 16 (RASS_ERR_UNSUPPORTED beyond). */
int rass_ivf_build_ex(rass_index_t* src, const float* centroids, int nlist,
                      const int32_t* assign, rass_dtype slab_dtype, rass_ivf_t** out);
void rass_ivf_destroy(rass_ivf_t* ivf);
/* IVF persistence (SURVEY §8f-3 for the IVF shard): the whole device state — list table, slab ids, tags,
 * centroid slab, permuted row slab — so a load needs neither the flat index nor a re-training.  The file is
 * fsynced before close (write to a temporary name and rename for crash safety, as docstore.py does). */
int rass_ivf_save(rass_ivf_t* ivf, const char* path);
int rass_ivf_load(rass_engine_t* eng, const char* path, rass_ivf_t** out);
int64_t rass_ivf_rows(const rass_ivf_t* ivf);
int rass_ivf_nlist(const rass_ivf_t* ivf);
int rass_ivf_dtype(const rass_ivf_t* ivf); /* rass_dtype of the row slab; -1 for NULL */
/* Same contract as rass_index_search; nprobe >= 1 lists per query, capped at nlist.
 * nprobe <= 32 probes the first nprobe lists by (centroid score desc, list id asc); nprobe > 32
 * probes every list whose coarse score is >= the nprobe-th best, so lists that tie with the
 * nprobe-th are all probed (tests/test_gpu_ivf_probe.py pins both rules).
 * *scanned_rows (may be NULL) receives the rows the fine scans touched. */
int rass_ivf_search(rass_ivf_t* ivf, const float* queries, int nq, int k,
                    int nprobe, const int32_t* q_filter, float* out_scores,
                    int64_t* out_ids, int64_t* scanned_rows);
int rass_ivf_search_device(rass_ivf_t* ivf, const float* d_queries, int nq,
                           int k, int nprobe, const int32_t* d_q_filter,
                           float* d_out_scores, int64_t* d_out_ids);
/* Up to 1 024 queries (32 launch groups) per call, device-resident: bit-identical to rass_ivf_search_device on
 * consecutive groups of 32 queries, with ONE normalise, ONE grouped coarse scan over the centroid slab, ONE plan launch
 * (the coarse lists are merged inside it) and ONE grouped merge for the whole batch — 4 + G launches instead of 5 G,
 * which is what an IVF probe at nprobe 1-2 (where two-level training puts recall 1.0) is bound by.  Outputs contiguous
 * [nq][k]; d_scanned_per_group (may be NULL): int64 per launch group, the rows its fine scan touched.  nprobe > 32 runs
 * group by group, and so does an IVF whose list masks and coarse candidates exceed the plan workgroup's LDS
 * (nlist + 64 * wpg * nprobe > 39 936 words, wpg = min(8, 256 / nprobe) coarse lists per query: above 23 552 lists at
 * nprobe 32).  (The reference's k-NN lookup under concurrent load: app/main.py:1552; BASELINE configs[4].) */
int rass_ivf_search_device_batch(rass_ivf_t* ivf, const float* d_queries, int nq, int k, int nprobe,
                                 const int32_t* d_q_filter, float* d_out_scores, int64_t* d_out_ids,
                                 int64_t* d_scanned_per_group);

/* ---- IVF + flat delta: the approximate index that stays incrementally insertable.
 * Replaces what the reference gets from OpenSearch's knn_vector field: an approximate (HNSW) index
 * (app/main.py:563-572) that takes bulk inserts of 64 docs at any time (app/main.py:1253-1282) and honours
 * `_id` overwrites / deletes.  Here: the IVF is a snapshot of source rows [0, covered); rows the source index
 * takes afterwards (the DELTA) are scanned exactly from its own slab in the same call and merged with the
 * probe's list by the same merge kernel; tombstones are honoured on both sides.
 *
 * rass_ivf_build_prefix: rass_ivf_build_ex over the first `n_rows` source rows only (-1 = all).  An IVF that
 * is to be searched with a delta must cover a multiple of 32 rows (the scan's tile), or every row.
 * rass_ivf_delete: tombstone source row `src_row` inside the IVF's slab (a no-op for rows it does not cover or
 * that are already gone) — call it next to rass_index_delete on the source index.
 * rass_ivf_search_delta[_device]: per query the exact top-k over (the rows of its nprobe best lists) U (source
 * rows >= covered), ties (score desc, source ordinal asc); ids = source ordinals, or the source index's
 * caller-assigned ids (rass_index_add_ex).  `q_filter` / `q_filter_mask` as rass_index_search_ex.  With
 * nprobe >= nlist the result equals rass_index_search_ex on the source index bit for bit (fp32 slab).
 * nq <= RASS_MAX_QBATCH for the device variant; k <= RASS_MAX_K (deeper lists: search the source index).
 * IVF files written since round 4 (versions 3 / 4) carry `covered`; older files load with covered = the
 * largest slab id + 1. */
int rass_ivf_build_prefix(rass_index_t* src, const float* centroids, int nlist,
                          const int32_t* assign, rass_dtype slab_dtype,
                          int64_t n_rows, rass_ivf_t** out);
int64_t rass_ivf_covered_rows(const rass_ivf_t* ivf);
int rass_ivf_delete(rass_ivf_t* ivf, int64_t src_row);
int rass_ivf_search_delta(rass_ivf_t* ivf, rass_index_t* src, const float* queries,
                          int nq, int k, int nprobe, const int32_t* q_filter,
                          const int32_t* q_filter_mask, float* out_scores,
                          int64_t* out_ids, int64_t* scanned_rows);
int rass_ivf_search_delta_device(rass_ivf_t* ivf, rass_index_t* src,
                                 const float* d_queries, int nq, int k, int nprobe,
                                 const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                 float* d_out_scores, int64_t* d_out_ids);

/* ---- The IVF probe WITHIN A ROW BITMAP: filtered k-NN that stays in the IVF.
 * rass_index_search_allowed streams every 32-row tile of the source in which a bitmap has a bit: cheap under a selective
 * filter, the whole slab under a broad one (a doc_type term, a year of dates, a must_not).  The reference's index filters
 * inside its approximate walk (OpenSearch k-NN with `filter`, app/main.py:563-572), choosing "exact over the filtered set" or
 * "ANN restricted to the set" by the size of the set; this is the second half.
 *
 * rass_ivf_search_allowed_delta[_device]: per query the exact top-k over ((the rows of its nprobe best lists) U (source rows
 * >= covered)) AND (the rows its bitmap allows), ties (score desc, source ordinal asc); ids = source ordinals, or the source
 * index's caller-assigned ids.  `allow`, n_bitmaps and words_per_bitmap as rass_index_search_allowed: uint32 words over SOURCE
 * row ordinals, one bitmap per query or one shared, words_per_bitmap >= ceil(rows / 32) of the source now; bits of tombstoned
 * rows, bits at or past the row count and surplus words allow nothing.  `q_filter` / `q_filter_mask` as rass_index_search_ex.
 * Scores are the flat scan's: with nprobe >= nlist the answer equals rass_index_search_allowed on the source bit for bit; at
 * any nprobe it equals rass_index_search_allowed with the bitmap restricted to the probed lists' rows and the delta.
 * Per launch group of RASS_MAX_QBATCH queries: the coarse stage and the plan of every probe; a kernel that reads, for every
 * planned tile, the bits of the source rows behind it (the slab is a permutation of the source) into slab-order words,
 * narrows each tile's query mask to the queries that still have a row in it and drops the tiles nobody has (order kept);
 * the allow-list scan over the slab on that work list; where the source holds rows behind `covered`, the allow-list scan
 * of those; the merge.  The words live in a workspace of the IVF ([32][tiles] uint32, allocated by the first such search).
 * *scanned_rows (host form; may be NULL) = the rows of the probe tiles kept + the rows of the delta tiles planned, summed
 * over the launch groups; *d_scanned_rows (device form; may be NULL) the same as one device int64.
 * 0 <= nq <= RASS_MAX_DEVICE_BATCH, group after group: the one-launch batch of rass_ivf_search_device_batch has no bitmap
 * form.  RASS_ERR_UNSUPPORTED: a bf16 or int8 slab (their scans have no bitmap mode), k > RASS_MAX_K (one pass, no
 * continuation: search the source index), dim > 1024.  RASS_ERR_INVALID: k or nprobe < 1, n_bitmaps neither 1 nor nq,
 * words_per_bitmap too small, a source compacted since the build.  Every refusal leaves both objects usable.
 * The device form is stream-ordered and synchronises nothing.
 *
 * rass_ivf_probe_lists: the coarse stage alone — out_list_ids (HOST) [nq][nprobe] int64, query q's nprobe best lists, best
 * first (centroid score desc, list id asc), -1 past min(nprobe, nlist).  1 <= nprobe <= RASS_MAX_K (deeper probes pick
 * their lists by a score threshold and keep no ranked list): RASS_ERR_UNSUPPORTED above.  For routing and for explaining a
 * probe: these are exactly the lists rass_ivf_search* and rass_ivf_search_allowed_delta probe at that nprobe. */
int rass_ivf_search_allowed_delta(rass_ivf_t* ivf, rass_index_t* src, const float* queries,
                                  int nq, int k, int nprobe,
                                  const uint32_t* allow, int n_bitmaps, int64_t words_per_bitmap,
                                  const int32_t* q_filter, const int32_t* q_filter_mask,
                                  float* out_scores, int64_t* out_ids, int64_t* scanned_rows);
int rass_ivf_search_allowed_delta_device(rass_ivf_t* ivf, rass_index_t* src, const float* d_queries,
                                         int nq, int k, int nprobe,
                                         const uint32_t* d_allow, int n_bitmaps, int64_t words_per_bitmap,
                                         const int32_t* d_q_filter, const int32_t* d_q_filter_mask,
                                         float* d_out_scores, int64_t* d_out_ids, int64_t* d_scanned_rows);
int rass_ivf_probe_lists(rass_ivf_t* ivf, const float* queries, int nq, int nprobe, int64_t* out_list_ids);

/* ---- IVF builds whose list plan runs on the GPU, and an IVF extended without retraining.
 * The list plan is the step between "every row has a list" and "the slab is filled": list lengths, tile-aligned
 * list offsets, the source row at every slab position and its inverse.  rass_ivf_build_prefix computes it in host
 * loops over all rows; here it is a stable counting sort on the device (csrc/ivf_build.hip), DEFINED to give what
 * those loops give.  No O(rows) host work, no id upload: per build the host reads 24 bytes (to size the slab) and
 * the row -> slab position map once (rass_ivf_delete reads it on the host).
 *
 * rass_ivf_plan_lists: the plan on caller-owned device arrays; stateless, ordered on `stream`.
 *   in : d_assign[n_rows] (the list of source row r), d_tags[n_rows] (RASS_ROW_TAG_DELETED = in no list), nlist in
 *        [1, 32768], tile_rows 32 or 64.
 *   out: d_list_len[nlist] live rows per list; d_list_tile0[nlist] the exclusive prefix of ceil(len / tile_rows);
 *        *d_total_tiles their sum (0 when no row is live); d_slab_ids[slab_rows], slab_rows = max(total_tiles, 1) *
 *        tile_rows: the source row at each slab position, ascending inside a list, -1 on padding; d_pos_of[n_rows]
 *        the slab position of each source row, -1 for a row in no list; *d_status: 0, or a sum of 1 (a live row's
 *        list id is outside [0, nlist): such rows are left out), 2 (total_tiles * tile_rows exceeds 0x7fffffc0:
 *        nothing is placed) and 4 (slab_rows exceeds slab_ids_capacity: nothing is written at or past it).
 *   d_workspace: rass_ivf_plan_workspace_bytes(n_rows, nlist) bytes (0 for arguments out of range).
 *   The output is a function of the input: atomics produce counts only, and no workgroup waits on another.
 * rass_ivf_build_device: rass_ivf_build_prefix with the assignment in device memory (what rass_kmeans_assign
 *   wrote); `centroids` stays a host array.  The same IVF, array by array (rass_ivf_save: the same bytes).
 * rass_ivf_absorb: a NEW IVF with the centroids, nlist and slab dtype of `ivf`, covering source rows [0, n_rows)
 *   (-1 = all): rows `ivf` covers keep their list, the rows after them go to their nearest centroid (as a build:
 *   ties to the lowest list), rows tombstoned since the build drop out.  The result is the IVF rass_ivf_build_prefix
 *   gives from those centroids and that assignment.  `ivf` is untouched and stays searchable; the caller destroys
 *   it.  Out of place, like rass_index_compact: the new IVF needs HBM next to the old one (RASS_ERR_OOM).
 *   RASS_ERR_INVALID: n_rows below rass_ivf_covered_rows(ivf), above the source's rows, or neither a multiple of
 *   32 nor all rows; a source compacted since the build.  RASS_ERR_UNSUPPORTED: a non-fp32 or wide-row source.
 *   Every refusal leaves *out = NULL and both inputs as they were.
 * rass_ivf_lists_device: the lists of an IVF (built, absorbed or loaded) as arrays: d_assign[covered] (may be
 *   NULL) the list of every covered source row in the slab, -1 for the others; d_list_len[nlist] (may be NULL).
 *   Returns with the copies complete. */
size_t rass_ivf_plan_workspace_bytes(int64_t n_rows, int nlist);
int rass_ivf_plan_lists(const int32_t* d_assign, const int32_t* d_tags, int64_t n_rows, int nlist,
                        int tile_rows, int32_t* d_list_len, int32_t* d_list_tile0,
                        int64_t* d_total_tiles, int64_t* d_slab_ids, int64_t slab_ids_capacity,
                        int32_t* d_pos_of, int32_t* d_status, void* d_workspace,
                        size_t workspace_bytes, void* stream);
int rass_ivf_build_device(rass_index_t* src, const float* centroids, int nlist,
                          const int32_t* d_assign, rass_dtype slab_dtype, int64_t n_rows,
                          rass_ivf_t** out);
int rass_ivf_absorb(rass_ivf_t* ivf, rass_index_t* src, int64_t n_rows, rass_ivf_t** out);
int rass_ivf_lists_device(rass_ivf_t* ivf, int32_t* d_assign, int64_t assign_capacity,
                          int32_t* d_list_len);

/* ---------------------------------------------------------------- encoder
 * Replaces ollama_embed_text / embed_texts_in_batches / embed_query's HTTP hop
 * to Ollama (app/main.py:225-274): a BERT-class post-LN sentence encoder
 * (mxbai-embed-large class, OLLAMA_EMBED_MODEL app/main.py:67) run as one
 * batched, varlen-packed forward of hand-written gfx950 kernels (bf16 MFMA
 * GEMMs with fused bias/GELU/residual epilogues, LDS-resident attention,
 * LayerNorm, pooling). */
typedef struct rass_encoder rass_encoder_t;

typedef struct rass_encoder_config {
    int32_t vocab_size;     /* 30522 */
    int32_t hidden;         /* 1024 = EMBED_DIM; must be heads * 64 */
    int32_t layers;         /* 24 */
    int32_t heads;          /* 16 */
    int32_t intermediate;   /* 4096 */
    int32_t max_positions;  /* <= 512 */
    int32_t pooling;        /* 0 = cls, 1 = mean over tokens */
    int32_t normalize;      /* != 0: L2-normalise the pooled vector, e/(||e||+1e-9) */
    float layer_norm_eps;   /* 1e-12 */
} rass_encoder_config;

int rass_encoder_create(int device, const rass_encoder_config* cfg,
                        rass_encoder_t** out);
void rass_encoder_destroy(rass_encoder_t* enc);
int rass_encoder_hidden(const rass_encoder_t* enc);
/* One call per tensor, by its Hugging Face BERT name ("embeddings.word_
 * embeddings.weight", "encoder.layer.7.attention.self.query.weight", ...),
 * fp32 host data in the checkpoint's layout ([out][in] for Linear). */
int rass_encoder_set_weight(rass_encoder_t* enc, const char* name,
                            const float* data, int64_t numel);
/* Checks that every tensor of the architecture was supplied. */
int rass_encoder_finalize(rass_encoder_t* enc);
/* token_ids: all sequences back to back (each already [CLS] ... [SEP],
 * <= max_positions tokens); cu_seqlens[nseq+1] prefix sums starting at 0.
 * out: nseq x hidden fp32, order = input order. */
int rass_encode(rass_encoder_t* enc, const int32_t* token_ids,
                const int32_t* cu_seqlens, int nseq, float* out);
/* Device-resident, asynchronous on `stream`.  NULL means the encoder's OWN
 * (non-blocking) stream, rass_encoder_get_stream() — NOT HIP's legacy null
 * stream, with which it does not synchronise.  The output can be handed
 * straight to rass_index_add_device when the engine runs on the same stream
 * (rass_engine_set_stream(eng, rass_encoder_get_stream(enc)), or one caller
 * stream passed to both); on different streams the caller must order them. */
int rass_encode_device(rass_encoder_t* enc, const int32_t* d_token_ids,
                       const int32_t* d_cu_seqlens, int nseq, int total_tokens,
                       int max_seqlen, float* d_out, void* stream);
/* The hipStream_t rass_encode() and rass_encode_device(stream = NULL) run on. */
void* rass_encoder_get_stream(rass_encoder_t* enc);
/* Counters since create: out[0] forwards launched (rass_encode + rass_encode_device), out[1] sequences, out[2]
 * tokens.  What the embed micro-batcher's tests read: N concurrent embed_query coroutines (app/main.py:2800, up to
 * MAX_EMBED_CONCURRENCY in flight, 250-260) must arrive as one or two forwards, not N. */
int rass_encoder_stats(rass_encoder_t* enc, int64_t out[3]);
/* The encoder's GEMM on its own: Y[m,n] = epi(X[m,k] W[n,k]^T + bias), bf16
 * operands; epilogue 0 bias, 1 bias+residual, 2 bias+GELU(erf).  m_pad
 * (multiple of 128) rows must be allocated; n % 128 == 0, k % 64 == 0. */
int rass_gemm_bf16(const void* d_x, const void* d_w, const float* d_bias,
                   const void* d_residual, void* d_y, int m, int m_pad, int n,
                   int k, int epilogue, void* stream);
/* Same with a caller-owned fp32 scratch (d_ws, ws_bytes >= 2 * m_pad * n * 4): a GEMM over few rows (m_pad <= 256)
 * is then split over K so that enough workgroups stream the weights — the path the encoder takes for embed_query /
 * ollama_embed_text (app/main.py:225-237, 266-274); slices are summed in fixed order (deterministic). */
int rass_gemm_bf16_ws(const void* d_x, const void* d_w, const float* d_bias,
                      const void* d_residual, void* d_y, int m, int m_pad, int n, int k,
                      int epilogue, void* d_ws, size_t ws_bytes, void* stream);
/* The encoder's self-attention on its own (what llama.cpp computes per layer behind the reference's POST to Ollama,
 * app/main.py:225-237): d_qkv bf16 [tokens][3*hidden] (q | k | v per token), sequences packed back to back with
 * d_cu_seqlens[nseq + 1] token offsets (total_tokens = the last one, as the host knows it), heads of 64
 * (hidden = 64 * heads), every sequence <= max_seqlen <= 512, softmax(q k^T / 8) v in fp32, d_ctx bf16
 * [total_tokens][hidden].  A sequence may be EMPTY (two equal offsets; the offsets live on the device, so the host
 * cannot refuse one as rass_encode does): it owns no rows of d_ctx and nothing is written for it, whichever kernel the
 * launch takes; the rows of its neighbours are what they are without it. */
int rass_attention_bf16(const void* d_qkv, const int32_t* d_cu_seqlens, int nseq, int total_tokens,
                        int max_seqlen, int hidden, int heads, void* d_ctx, void* stream);
/* Query time (embed_query / ollama_embed_text, app/main.py:225-237, 266-274: one text, a dozen tokens): the attention and
 * the attention-output projection in ONE launch — d_y = attention(d_qkv) d_w^T + d_bias + d_residual, d_w bf16 [n][hidden],
 * d_residual / d_y bf16 [total_tokens][n].  Every workgroup of the projection recomputes the attention (its context rows
 * have rass_attention_bf16's bits); a launch of a one-query forward costs 4-5 us whatever it does, this saves one per layer.
 * 1 <= total_tokens <= 32 over all nseq sequences, hidden = 1024, heads = 16, n % 16 == 0; anything else (or
 * RASS_ATTN_FUSE=0 in the environment) -> RASS_ERR_UNSUPPORTED.  rass_encode_device takes it by itself. */
int rass_attention_out_bf16(const void* d_qkv, const int32_t* d_cu_seqlens, int nseq, int total_tokens, int hidden,
                            int heads, const void* d_w, const float* d_bias, const void* d_residual, void* d_y, int n,
                            void* stream);
/* The encoder's other kernels on their own (tests): each is one launch, or the pair of launches, a forward makes, with the
 * forward's own dispatch and A/B switches (RASS_LN_*, RASS_GEMM_*, read at every call).  Activations are bf16 row-major,
 * LayerNorm parameters, biases and statistics fp32; row kernels take hidden % 8 == 0, hidden <= 2048 (else
 * RASS_ERR_UNSUPPORTED).  A launcher's refusal of a shape is RASS_ERR_INVALID. */
/* Embedding + LayerNorm: out[t] = LayerNorm(word[ids[t]] + pos[p] + type0) for the total_tokens tokens packed by
 * d_cu_seqlens[nseq + 1], p = t's position in its sequence.  An id < 0 or >= vocab reads row 0; p >= max_pos reads row
 * max_pos - 1.  word [vocab][hidden], pos [max_pos][hidden], type0 [hidden] bf16; out [total_tokens][hidden]. */
int rass_embed_layernorm_bf16(const int32_t* d_ids, const int32_t* d_cu_seqlens, int nseq, int total_tokens, const void* d_word,
                              const void* d_pos, const void* d_type0, const float* d_gamma, const float* d_beta, float eps,
                              int hidden, int vocab, int max_pos, void* d_out, void* stream);
/* LayerNorm of `rows` rows: out = (x - mean) * rsqrt(var + eps) * gamma + beta, fp32 two-pass statistics, bf16 out.
 * From 4 096 rows on the loads are nontemporal (RASS_LN_NT: bit 0 loads, bit 1 stores); the bits do not depend on it. */
int rass_layernorm_bf16(const void* d_in, const float* d_gamma, const float* d_beta, float eps, int rows, int hidden,
                        void* d_out, void* stream);
/* out = LayerNorm(bf16(x w^T + bias + residual)), the attention-output / FFN-down step: x [m_pad][k], w [n][k], residual,
 * y, out [m_pad][n].  d_ws == NULL: the GEMM (epilogue 1) into y, then rass_layernorm_bf16 of y.  With an fp32 scratch the
 * encoder's own choice for m: few rows take the one-launch GEMM (K of 4 096: four K slices and one reduce + residual +
 * LayerNorm launch), mid-size ones split K with the reduction fused into the LayerNorm (y is then not written).
 * `residual` may be `out`.  Rows m .. m_pad - 1 of y and out are not written. */
int rass_gemm_bf16_residual_layernorm(const void* d_x, const void* d_w, const float* d_bias, const void* d_residual, void* d_y,
                                      const float* d_gamma, const float* d_beta, float eps, void* d_out, int m, int m_pad, int n,
                                      int k, void* d_ws, size_t ws_bytes, void* stream);
/* A query's FFN-up: y = epi(LayerNorm(yin) w^T + bias), epilogue 0 bias / 2 bias + GELU(erf), with the LayerNorm's rows
 * (the bits rass_layernorm_bf16 writes) also stored to x_out.  1 <= m <= 32, k = 1024, n % 16 == 0, n >= 1024, else
 * RASS_ERR_UNSUPPORTED.  yin, x_out [m][1024], y [m][n]. */
int rass_gemm_bf16_ln_input(const void* d_yin, const float* d_gamma, const float* d_beta, float eps, void* d_x_out, const void* d_w,
                            const float* d_bias, void* d_y, int m, int n, int k, int epilogue, void* stream);
/* LayerNorm folded into its consumer's weights: w2[n][k] = bf16(w[n][k] * gamma[k]), colsum[n] = sum_k w2[n][k] (fp32),
 * bias2[n] = bias[n] + sum_k beta[k] * w[n][k]. */
int rass_fold_gamma_bf16(const void* d_w, const float* d_gamma, const float* d_beta, const float* d_bias, int n, int k, void* d_w2,
                         float* d_colsum, float* d_bias2, void* stream);
/* The GEMMs of the folded-LayerNorm forward (big batches).  mr [m][2] holds a (mean, rstd) per row.  Epilogue 3:
 * y = bf16(x w^T + bias + LN(residual_raw)), LN rebuilt from (mr, gamma, beta), and stats [m][n / 128][2] receives each
 * 128-column chunk's (sum, sum of squares) of the stored y.  Epilogue 4 / 5: y = rstd * (x w2^T - mean * colsum) + bias2
 * [+ GELU], from rass_fold_gamma_bf16's outputs.  m >= 1024, m_pad % 256 == 0, n % 256 == 0, k % 64 == 0, k >= 128 and
 * >= 192 tiles of 256 x 256, else RASS_ERR_UNSUPPORTED.  Rows m .. m_pad - 1 of y are not written. */
int rass_gemm_bf16_fold(const void* d_x, const void* d_w, const float* d_bias, const void* d_residual_raw, void* d_y, int m,
                        int m_pad, int n, int k, int epilogue, const float* d_mr, const float* d_gamma, const float* d_beta,
                        float* d_stats, const float* d_colsum, void* stream);
/* Which kernel a GEMM entry point would take for this shape, as a short label written into `label` (NUL-terminated, cut to
 * label_bytes): entry 0 = rass_gemm_bf16_ws (epilogue 0 / 1 / 2), 1 = rass_gemm_bf16_residual_layernorm, 2 =
 * rass_gemm_bf16_ln_input (epilogue 0 / 2), 3 = rass_gemm_bf16_fold (epilogue 3 / 4 / 5); ws_bytes = 0: no scratch lent.
 * Labels: fewrows4, fewrows16, splitk<S>, mid64, mid128, tile128, p4, p5; residual_layernorm: fewrows4+ln, splitk<S>+ln,
 * fewrows+pair, pair; ln_input: lnin16, lnin4; and "unsupported".  Stateless: it touches no device and needs none; it reads
 * the RASS_GEMM_* switches of the environment as a launch would. */
int rass_gemm_bf16_route(int entry, int m, int m_pad, int n, int k, int epilogue, size_t ws_bytes, char* label, size_t label_bytes);
/* stats [rows][n / 128][2] of epilogue 3 -> mr [rows][2] = (mean, rsqrt(var + eps)), summed in chunk order. */
int rass_ln_stats_finalize(const float* d_stats, int rows, int n, float eps, float* d_mr, void* stream);
/* Pooling: out[s] = the mean over sequence s's tokens (mode_mean) or its first token, fp32 [nseq][hidden]; normalize:
 * e / (||e|| + 1e-9).  An empty sequence gives zeros. */
int rass_pool_bf16(const void* d_x, const int32_t* d_cu_seqlens, int nseq, int hidden, int mode_mean, int normalize,
                   float* d_out, void* stream);

/* -------------------------------------------------------------- tokenizer
 * BERT (uncased) BasicTokenizer + WordPiece on the host (C++), replacing the
 * tokenisation Ollama / llama.cpp performs on every chunk the reference posts
 * (app/main.py:225-237): lower-case, NFD + accent strip, punctuation split,
 * CJK spacing, greedy longest-match-first pieces, [CLS] ... [SEP], truncated
 * to max_len.  Unicode tables are generated from Python's unicodedata. */
typedef struct rass_tokenizer rass_tokenizer_t;
int rass_tokenizer_create(const char* vocab_path, int lower_case,
                          rass_tokenizer_t** out);
void rass_tokenizer_destroy(rass_tokenizer_t* tok);
int rass_tokenizer_vocab_size(const rass_tokenizer_t* tok);
/* Returns the number of ids written (<= max_len) or a negative status. */
int rass_tokenizer_encode(const rass_tokenizer_t* tok, const char* text,
                          int64_t text_len, int max_len, int32_t* out_ids);
/* n UTF-8 texts -> packed ids (capacity n*max_len) + cu_seqlens[n+1], fanned
 * out over n_threads (<= 0: all cores).  Returns the total token count. */
int64_t rass_tokenizer_encode_batch(const rass_tokenizer_t* tok,
                                    const char* const* texts,
                                    const int64_t* lens, int n, int max_len,
                                    int32_t* out_ids, int32_t* out_cu,
                                    int n_threads);

/* HIP-event timing on an explicit stream (bench.py measures kernels on the
 * stream they run on; torch.cuda.Event only sees torch's current stream). */
typedef struct rass_timer rass_timer_t;
int rass_timer_create(rass_timer_t** out);
void rass_timer_destroy(rass_timer_t* t);
int rass_timer_start(rass_timer_t* t, void* stream);
int rass_timer_stop(rass_timer_t* t, void* stream);
/* Blocks until the stop event has completed; milliseconds between the two. */
int rass_timer_elapsed_ms(rass_timer_t* t, float* ms);

/* Bracket every scan-kernel launch the engine makes with a hipEvent pair on
 * the engine stream (up to max_launches launches), then read back the summed
 * kernel time: bench.py's live per-kernel duration for the roofline figure.
 * `launches` counts launch GROUPS of <= RASS_MAX_QBATCH queries: a batch call's 64-query corpus pass, which serves
 * two groups in one kernel launch, counts as two (its time is summed once). */
int rass_engine_kernel_timing_begin(rass_engine_t* eng, int max_launches);
int rass_engine_kernel_timing_end(rass_engine_t* eng, double* total_ms,
                                  int* launches);

/* Device pointers of an index's tile16 slab / tag array (zero-copy interop,
 * e.g. rass_scan_topk_f32 over a row prefix).  Invalidated by growth. */
void* rass_index_device_rows(rass_index_t* idx);
void* rass_index_device_tags(rass_index_t* idx);

/* Name of the scan kernel variant a (dim, nq) request dispatches to, for
 * matching rocprofv3 kernel-trace rows ("" if unsupported). */
const char* rass_scan_kernel_name(int dim, int nq);

#ifdef __cplusplus
}
#endif
#endif /* RASS_ENGINE_H */
