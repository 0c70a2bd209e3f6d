/*
 * vsearch.h — C-ABI of libvsearch.so, the MI355X-native exact flat-index engine.
 *
 * This is the drop-in boundary for the reference's one data-parallel hot path:
 * brute-force top-k over 1536-d book / student embeddings.  In the reference the
 * path is reached through LangChain's `FAISS` vector store
 * (langchain-community 0.3.26, /root/reference/poetry.lock:1577-1578) whose
 * `.index` is a faiss-cpu 1.11.0 `IndexFlatL2` / `IndexFlatIP`
 * (/root/reference/poetry.lock:866-867), plus the pgvector cosine top-15
 * self-join in /root/reference/src/graph_refresher/main.py:339-354.
 *
 * Every entry point below names the reference interface it replaces.  faiss and
 * langchain are not vendored in /root/reference; their call sites are cited.
 *
 * Conventions
 *   - every function returns 0 on success, a negative VS_E* code on failure;
 *     the message is available from vs_last_error() (thread-local).
 *   - vectors are C-contiguous float32 rows of length d (what faiss's SWIG layer
 *     receives after np.ascontiguousarray(x, dtype="float32")).
 *   - `flags` say where caller buffers live (VS_IN_DEVICE / VS_OUT_DEVICE);
 *     device buffers must be on the index's device.
 *   - `stream` is a hipStream_t (NULL = the legacy default stream).  Calls with
 *     host outputs synchronise that stream before returning.
 *   - labels are int64, exactly faiss's idx_t; padding label is -1.
 */
#ifndef VSEARCH_H
#define VSEARCH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Metric codes equal faiss::MetricType so index.metric_type passes straight through. */
#define VS_METRIC_INNER_PRODUCT 0
#define VS_METRIC_L2 1

/* Storage dtype of the database rows. */
#define VS_DTYPE_F32 0
#define VS_DTYPE_BF16 1

/* Buffer-location flags. */
#define VS_IN_DEVICE 1  /* input vectors / ids are device pointers */
#define VS_OUT_DEVICE 2 /* output buffers are device pointers      */
/* vs_search: return the k entries with the lexicographically smallest
 * (key, label), key = distance (L2) or -score (IP), in that order, instead of
 * faiss's inner-product tie order.  The per-shard half of an exact row-sharded
 * search: faiss's IP tie rule is a function of the 2k-1 best (key, label) pairs
 * of the union, so each shard returns its raw best 2k-1 (any k) and
 * vs_merge_topk applies the rule once (vsearch/sharded.py).  No effect on L2. */
#define VS_RAW_ORDER 4
/* vs_search_where: skip the windows and answer every query with the
 * predicated scan. */
#define VS_WHERE_SCAN 8
/* vs_search_boost: skip the windows and answer every query with the boosted
 * scan. */
#define VS_BOOST_SCAN 16   /* skip the windows */

/* Status codes. */
#define VS_OK 0
#define VS_E_INVALID (-1) /* bad argument (faiss: FAISS_THROW_IF_NOT / assert) */
#define VS_E_HIP (-2)     /* HIP runtime / launch error                        */
#define VS_E_OOM (-3)     /* device allocation failed                          */
#define VS_E_UNSUPPORTED (-4)

/* The entries one exact page holds (register lists of 64).  Not a limit on k:
 * searches and self-joins that need more — k > 64, raw k > 64, faiss's
 * inner-product tie rule at k > 32 — read further pages of 64, each after the
 * previous page's last (key, label) (vs_engines.hip run_paged), as faiss-cpu's
 * IndexFlat::search answers any k. */
#define VS_MAX_K 64

typedef struct vs_index vs_index;

/* Thread-local text of the last error (faiss: FaissException::what()). */
const char* vs_last_error(void);
/* Library ABI version (major*10000 + minor*100 + patch). */
int vs_version(void);
/* Number of visible HIP devices. */
int vs_device_count(int* n);

/* ---- index lifetime -------------------------------------------------------
 * Replaces faiss.IndexFlatL2(d) / faiss.IndexFlatIP(d), created by
 * FAISS.from_texts (default EUCLIDEAN => IndexFlatL2) at
 * src/ingestion_service/pipeline.py:359, src/incremental_workers/book_vector/main.py:121,469,
 * src/recommendation_api/candidate_builder.py:69-71, src/recommendation_api/service.py:370-372. */
int vs_create(int d, int metric, int dtype, int device, vs_index** out);
int vs_destroy(vs_index* idx);

/* Pre-size device storage for n rows (no faiss equivalent; avoids regrowth copies). */
int vs_reserve(vs_index* idx, int64_t n);

/* faiss Index::add(n, x) — appends rows; labels continue at ntotal.
 * Callers: FAISS.add_texts at src/ingestion_service/pipeline.py:363,
 * src/incremental_workers/book_vector/main.py:148. */
int vs_add(vs_index* idx, const float* x, int64_t n, int flags, void* stream);

/* In-place update: the live row with label labels[i] takes the value x[i]
 * (n * d float32), exactly as if that value had been added there: fp32 indexes
 * store the bits given, bf16 indexes the round-to-nearest-even value vs_add
 * would store, and every derived byte (norms, filter planes, scales, residual
 * and augmented norms) is the one vs_add derives.  Replaces remove-then-add
 * for the reference's upserts (student_embedding/main.py:137-145 ON CONFLICT
 * DO UPDATE; the re-embedding of a book, book_vector/main.py:148).
 *
 * labels is HOST int64 (id_base applied); VS_IN_DEVICE covers x only.  A label
 * is mapped to its row in place through the tombstone list, so an index with
 * unpacked removals works.  Checked before anything is written, in this order
 * (on failure the index is unchanged): the index, n >= 0, the buffers; every
 * label is a live label (VS_E_INVALID otherwise, the labels faiss reconstruct
 * throws for); no label is given twice (VS_E_INVALID).  n == 0 is success.
 *
 * No row moves and no label changes, so the index's generation stays: a
 * selector or a grouping built before the call stays valid and sees the new
 * values.  The call waits for the searches of this index already enqueued
 * (as a storage growth in vs_add does) and returns after `stream` is
 * synchronised, as vs_add: the caller may free x.  Its cost does not depend on
 * the rows the index holds (but for the O(removed) walk that maps labels).
 *
 * The bound maxima of the filter planes only grow here: they may stay higher
 * than a fresh index's until vs_remove_ids recomputes them.  A maximum that is
 * too high is still a bound: results do not change, only how early a query is
 * settled. */
int vs_update_rows(vs_index* idx, const int64_t* labels, const float* x, int64_t n, int flags,
                   void* stream);

/* Appends n rows of the deterministic counter-based synthetic corpus
 * (row r = global row row0 + i; see vs_fill_synthetic).  Benchmark/test feed only. */
int vs_add_synthetic(vs_index* idx, int64_t n, uint64_t seed, int64_t row0, void* stream);

/* Appends n rows whose synthetic generator row numbers are ids[0..n) (host int64
 * array): row j of the append equals row ids[j] of vs_fill_synthetic's corpus.
 * Lets a benchmark rebuild any mutated corpus exactly.  Benchmark/test feed only. */
int vs_add_synthetic_ids(vs_index* idx, const int64_t* ids, int64_t n, uint64_t seed,
                         void* stream);

/* faiss Index::reset(). */
int vs_reset(vs_index* idx);

/* faiss Index::ntotal / ::d / ::metric_type (read at book_vector/main.py:162-170,
 * ingestion_service/pipeline.py:186,524). */
int vs_ntotal(const vs_index* idx, int64_t* out);
int vs_dim(const vs_index* idx, int* out);
int vs_metric(const vs_index* idx, int* out);
int vs_dtype(const vs_index* idx, int* out);

/* Arithmetic engine of the large-batch path of fp32 indexes:
 *   VS_ENGINE_AUTO          library default where it applies (IP k <= 28, L2 /
 *                           cosine k <= 56), else FP32_MFMA: filter and verify
 *                           in stages over the index's filter planes — int8
 *                           (inner product and cosine), then bf16 for the
 *                           queries the int8 bound cannot settle, then the exact
 *                           FP32_MFMA for what remains;
 *                           env VS_ENGINE=fp32|bf16v|i8v overrides
 *   VS_ENGINE_FP32_MFMA     v_mfma_f32_32x32x2_f32 on the fp32 rows
 *   VS_ENGINE_I8_VERIFY     filter and verify on the int8 plane alone: one int8
 *                           MFMA product per fp32 product (int8 codes of rows
 *                           and queries, one scale per row) keeps the best
 *                           candidates of every query, a rigorous error bound
 *                           proves the exact top-k is among them, the candidates
 *                           are rescored exactly, and queries the bound cannot
 *                           settle are redone by FP32_MFMA — results identical to
 *                           an exact engine
 *   VS_ENGINE_BF16_VERIFY   the same on the bf16 (round-to-nearest-even) plane
 * New fp32 indexes hold the int8 plane (inner product) and the bf16 plane;
 * env VS_FILTER=bf16|i8 at creation keeps one.  bf16 indexes ignore the
 * setting (bf16 MFMA on the stored values). */
#define VS_ENGINE_AUTO 0
#define VS_ENGINE_FP32_MFMA 1
#define VS_ENGINE_BF16_VERIFY 3
#define VS_ENGINE_I8_VERIFY 4
int vs_set_engine(vs_index* idx, int engine);

/* The filter planes an fp32 index holds, a bit set: VS_FILTER_I8 (int8 codes +
 * per-row scale; inner-product indexes) | VS_FILTER_BF16; 0 for bf16 indexes.
 * Library-specific (faiss has no counterpart); the benchmark reads it to price
 * the filter pass. */
#define VS_FILTER_I8 1
#define VS_FILTER_BF16 2
int vs_filter_plane(const vs_index* idx, int* out);
/* The last notice of the index: a filter plane dropped because HBM ran short
 * while the storage grew (searches stay exact on the plane that remains or the
 * exact fp32 engine, but slower); "" if none.  Library-specific.  The pointer
 * stays valid until the next mutation of the index. */
const char* vs_notice(const vs_index* idx);

/* Rows [0,ntotal) get labels id_base + row.  Used by the row-sharded multi-GPU
 * index so that per-shard results carry global faiss labels. */
int vs_set_id_base(vs_index* idx, int64_t id_base);

/* faiss IndexFlat::search(n, x, k, D, I) (knn_L2sqr / knn_inner_product):
 * exact top-k, D ascending squared-L2 or descending inner product, k > ntotal
 * padded with (+FLT_MAX | -FLT_MAX, -1).  Ties follow faiss's heaps: L2 keeps the
 * lower label first; inner product follows faiss's CMin-heap rule (equal scores
 * come out in DESCENDING label order, and which tied labels stay depends on the
 * labels of the better rows — vs_support.hip faiss_ip_tie_order, exact for
 * every k: the rule reads up to the 2k-1 best entries, taken from further
 * pages where the k-th key's run of equal keys fills a page).  Any k > 0
 * (k > ntotal pads; k > INT_MAX/2: VS_E_INVALID).  L2 calls with n < 20 use faiss's sequential branch (direct sum of
 * squares), n >= 20 the BLAS branch (|q|^2 + |x|^2 - 2 q.x clamped at 0).
 * Stream-ordered on `stream` when every buffer is on the device; the call
 * returns once its first filter stage's count of unsettled queries is known
 * (a 4-byte read; later stages are enqueued only for queries left; env
 * VS_TAIL_WAIT=0 or a capturing stream: fully asynchronous, every launch kept).
 * Caller: FAISS.similarity_search_with_score_by_vector, reached from
 * src/recommendation_api/mcp_book_server.py:142, candidate_builder.py:187,321,
 * service.py:529,627.  D is n*k float32, I is n*k int64. */
int vs_search(vs_index* idx, const float* x, int64_t n, int64_t k, float* D, int64_t* I,
              int flags, void* stream);

/* ---- selector searches -----------------------------------------------------
 * faiss index.search(x, k, params=SearchParameters(sel=IDSelector...)): the k
 * nearest rows among the selected labels only.  Replaces the reference's
 * over-fetch-then-drop loops (search k * 2, drop the books a student has read:
 * src/recommendation_api/candidate_builder.py:187-203, service.py:529-542,
 * 627-640) and LangChain's host-side `filter=` over fetch_k rows
 * (candidate_builder.py:150-153), which return fewer than k when the nearest
 * rows are mostly excluded.
 *
 * A selector belongs to one index and is reusable across searches.  bitmap is
 * HOST bytes in faiss's IDSelectorBitmap layout: label l is selected iff bit
 * ((l - id_base) & 7) of byte ((l - id_base) >> 3) is set; nbits bits are
 * given, labels past nbits or past ntotal are not selected.  Anything that
 * moves rows or changes labels (vs_add, vs_remove_ids, vs_reset,
 * vs_set_id_base to another base) makes the selector stale.  vs_update_rows
 * does neither: a selector stays valid across it. */
typedef struct vs_selector vs_selector;
int vs_selector_create(vs_index* idx, const uint8_t* bitmap, int64_t nbits, void* stream,
                       vs_selector** out);
/* The selected live rows. */
int vs_selector_count(const vs_selector* sel, int64_t* out);
int vs_selector_destroy(vs_selector* sel);
/* vs_search restricted to the selector's rows: same outputs, padding (fewer
 * than k selected rows pad with (+FLT_MAX | -FLT_MAX, -1)), tie rules (over the
 * selected rows only), flags (VS_IN_DEVICE / VS_OUT_DEVICE / VS_RAW_ORDER) and
 * stream contract.  A selector built before the index last changed:
 * VS_E_INVALID ("stale selector").  Selections that leave at most 256 live rows
 * out run the unselected engine for k plus the excluded rows and drop those
 * (any k); every other selection runs the gathered kernels over the selected
 * rows alone, one exact page: inner product k <= 32, L2 / VS_RAW_ORDER k <= 64,
 * VS_E_UNSUPPORTED past it.  L2 on the gathered streaming kernel (calls of at
 * most 32 queries) is faiss's sequential sum (x - q)^2 — the branch faiss-cpu
 * 1.11 takes for a search with a selector (distances.cpp knn_L2sqr, as
 * recalled: faiss is not vendored); larger calls use |q|^2 + |x|^2 - 2 q.x. */
int vs_search_sel(vs_index* idx, const vs_selector* sel, const float* x, int64_t n, int64_t k,
                  float* D, int64_t* I, int flags, void* stream);

/* ---- profile searches ------------------------------------------------------
 * The reference's per-student candidate path (reconstruct the embeddings of
 * the books a student rated, take their weighted mean, search k * 2, drop the
 * books already read: src/recommendation_api/candidate_builder.py:138-203,
 * service.py:490-542, 627-640) for many students in one call: every query has
 * its own exclusion list, and the queries can be built on the device from
 * stored rows.
 *
 * vs_search with one exclusion list per query.  excl_offs: n + 1 HOST int64
 * offsets, non-decreasing from 0; query q excludes the labels
 * excl_labels[excl_offs[q] .. excl_offs[q + 1]) (HOST int64).  Duplicates, -1
 * and labels that are not live labels of the index are ignored, as
 * vs_remove_ids ignores them.  Outputs, padding (fewer than k allowed rows pad
 * with (+FLT_MAX | -FLT_MAX, -1)), tie rules (over the allowed rows only),
 * VS_OUT_DEVICE, VS_RAW_ORDER, any k and the stream contract are vs_search's;
 * VS_IN_DEVICE applies to x only; the L2 formula follows the whole call's n.
 * excl_offs == NULL or all lists empty: vs_search itself.
 * Queries are grouped by the size m of their list (0; at most 16, 64, 256,
 * 1024; larger), and a group whose longest list holds c rows runs the engine
 * for k2 = min(need + c, live rows) raw entries (need = 2k - 1 for inner
 * product under faiss's tie rule, k otherwise) before its excluded rows are
 * dropped; groups the engine would serve with the same list length run as one.
 * So a query costs what its own group's longest list costs, not the call's:
 * k2 > 1024 leaves the staged engine for the paged one (k2 / 64 passes over
 * the rows), and k2 > INT_MAX/2 is VS_E_INVALID. */
int vs_search_excl(vs_index* idx, const float* x, int64_t n, int64_t k, const int64_t* excl_offs,
                   const int64_t* excl_labels, float* D, int64_t* I, int flags, void* stream);
/* n weighted means of stored rows: profile q is the labels
 * labels[offs[q] .. offs[q + 1]) with weights weights[...] (HOST CSR; offs:
 * n + 1 int64 from 0).  out: n * d float32, host or (VS_OUT_DEVICE) device.
 * Computed on the device in fp32, in list order, without FMA:
 *   acc = x[l0] * w0;  acc = fl(acc + fl(x[li] * wi));  out = fl(acc / W)
 * W = the weights summed in double in list order, rounded once to fp32; the
 * division is correctly rounded — numpy's np.sum([emb_i * w_i], axis=0) /
 * total_weight (candidate_builder.py:170-176) bit for bit for float32 rows.
 * bf16 indexes use the stored value widened to fp32, as vs_reconstruct_n
 * returns it.  VS_E_INVALID: a label that is not a live label (faiss
 * reconstruct throws), an empty profile, W zero or not finite. */
int vs_mean_rows(vs_index* idx, const int64_t* offs, const int64_t* labels, const float* weights,
                 int64_t n, float* out, int flags, void* stream);
/* Both in one call: the means of vs_mean_rows (kept on the device) searched as
 * vs_search_excl searches them.  excl_offs may be NULL; exclude_profile != 0
 * adds every profile's own labels to its exclusion list (the rated books are
 * the mean's nearest rows; the reference's already_read set holds them).
 * flags: VS_OUT_DEVICE, VS_RAW_ORDER. */
int vs_search_profiles(vs_index* idx, const int64_t* offs, const int64_t* labels,
                       const float* weights, int64_t n, int64_t k, const int64_t* excl_offs,
                       const int64_t* excl_labels, int exclude_profile, float* D, int64_t* I,
                       int flags, void* stream);

/* ---- distinct searches -----------------------------------------------------
 * The k nearest GROUPS, one best row per group (Qdrant search_groups with
 * group_size 1, Elasticsearch collapse, Milvus group_by_field).  The reference
 * appends a second row when a book is re-embedded
 * (src/incremental_workers/book_vector/main.py:148,
 * src/ingestion_service/pipeline.py:363), and its callers search k * 2 and
 * skip the book ids they have seen
 * (src/recommendation_api/candidate_builder.py:512, service.py:387-399): a
 * book with many rows near the query swallows any fixed over-fetch.
 *
 * A grouping gives every label of an index a group: an int32 >= 0, or -1 for
 * "this row is its own group".  group_of_label: n HOST int32, entry i the group
 * of label id_base + i; n must equal the live row count (vs_ntotal), a value
 * below -1 is VS_E_INVALID (checked before the index is read).  The handle
 * keeps a device copy and the index's generation: whatever moves rows or
 * changes labels (vs_add, vs_remove_ids, vs_reset, a pack, vs_set_id_base to
 * another base) makes it stale.  vs_update_rows does neither: a grouping
 * stays valid across it. */
typedef struct vs_grouping vs_grouping;
int vs_grouping_create(vs_index* idx, const int32_t* group_of_label, int64_t n, void* stream,
                       vs_grouping** out);
/* The distinct groups, every -1 row counted as one. */
int vs_grouping_groups(const vs_grouping* grp, int64_t* out);
int vs_grouping_destroy(vs_grouping* grp);
/* For query q take the rows a plain search would rank (the live rows minus q's
 * exclusion list, excl_offs / excl_labels as vs_search_excl, NULL: none) in
 * VS_RAW_ORDER: ascending (key, label), key = distance or -score.  A group's
 * representative is its first row in that order: the best key, the lowest
 * label among equal keys.  The call returns what vs_search would return on an
 * index that held only the representatives: faiss's order over them (the
 * inner-product tie rule unless VS_RAW_ORDER), min(k, groups among the allowed
 * rows) entries, then (+FLT_MAX | -FLT_MAX, -1) padding; D is the
 * representative's score as vs_search reports it.  With every row its own
 * group the result is vs_search's.
 *
 * Exact for any grouping: a query is searched in raw order for a window of w
 * entries; if those hold `need` groups (2k - 1 under the inner-product rule,
 * else k) their first entries are the `need` best representatives, if they
 * hold fewer groups but every allowed row there are no more, otherwise the
 * query alone is searched again with a window four times longer, at last over
 * every live row (vs_distinct_plan shows the schedule).  A grouping where one
 * group holds most of a query's nearest rows pays for the long windows: past
 * 1,023 entries the paged engine answers, about w / 64 passes over the rows.
 *
 * Checked before the index is read, in this order: the index, the grouping,
 * n >= 0, k > 0 (VS_E_INVALID); k > 1024: VS_E_UNSUPPORTED (the collapse's
 * table holds 2 x 2047 groups); the exclusion offsets; the buffers.  A grouping
 * of another index or an older generation: VS_E_INVALID ("stale grouping").
 * flags: VS_RAW_ORDER, VS_IN_DEVICE (x), VS_OUT_DEVICE (D, I).  The call reads
 * a 4-byte count after every round but the last, so it waits for `stream`; a
 * capturing stream: VS_E_UNSUPPORTED. */
int vs_search_distinct(vs_index* idx, const vs_grouping* grp, const float* x, int64_t n, int64_t k,
                       const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                       int flags, void* stream);
/* Diagnostic (touches no device): the windows of a distinct search for k over
 * `live` rows, round by round: out[r] for r < nmax; non-decreasing, the last
 * one equal to `live`.  Returns the number of rounds of the whole schedule
 * (0 for live == 0), or VS_E_INVALID (k outside 1 .. 1024, a bad metric,
 * live < 0). */
int vs_distinct_plan(int64_t k, int metric, int raw, int64_t live, int64_t* out, int nmax);
/* Process-wide counters of the distinct searches since the last reset
 * (reset != 0 clears them): queries searched, rounds run (summed over the
 * calls' chunks of queries), and queries whose first window was too short
 * (searched again at least once). */
int vs_distinct_stats(int64_t* searches, int64_t* rounds, int64_t* requeried, int reset);

/* ---- where searches --------------------------------------------------------
 * Exact top-k under a predicate that differs per query (pgvector WHERE, Qdrant
 * payload filters, Milvus expr).  The reference conditions every
 * recommendation on the reader — a reading level band, genres
 * (src/recommendation_api/scoring.py:81-93, candidate_builder.py:187-203,
 * mcp_book_server.py:615-682) — and filters an over-fetch of k * 2 on the host
 * (service.py:529-542), which returns fewer than k once the predicate is
 * selective.
 *
 * An attribute handle gives every label of an index up to four float32
 * columns and one 64-bit tag word.  cols: HOST float32, column-major
 * [ncol][n], ncol in 0 .. 4; tags: HOST uint64 [n] or NULL (all 0); entry i
 * belongs to label id_base + i; n must equal the live row count.  A NaN
 * column value means "unknown".  The handle keeps the attributes on the
 * device by label and by row in place (one array when the index holds no
 * tombstones) and the index's generation: whatever moves rows or changes
 * labels (vs_add, vs_remove_ids, vs_reset, a pack, vs_set_id_base to another
 * base) makes it stale ("stale attributes"); it stays valid across
 * vs_update_rows.  Checked in this order: the output, the index, ncol, n, the
 * columns, then n against the live rows. */
typedef struct vs_attrs vs_attrs;
int vs_attrs_create(vs_index* idx, int ncol, const float* cols, const uint64_t* tags, int64_t n,
                    void* stream, vs_attrs** out);
int vs_attrs_destroy(vs_attrs* attrs);
/* The predicate of query q, from HOST arrays any of which may be NULL ("no
 * test"):
 *   lo, hi: float32 [nq][ncol].  Column c is tested unless lo == -inf and
 *           hi == +inf; a tested column passes iff lo <= v && v <= hi, so a NaN
 *           value fails it.  A NaN bound: VS_E_INVALID.
 *   masks:  uint64 [nq][3] = any_of, all_of, none_of: any_of == 0 ||
 *           (tags & any_of), (tags & all_of) == all_of, (tags & none_of) == 0.
 * A row passes iff every test passes; lo > hi matches nothing (legal).
 *
 * vs_attrs_count: out[q] (HOST int64 [nq]) = the live rows that pass predicate
 * q; one streaming kernel over the by-row arrays.  Waits for `stream`. */
int vs_attrs_count(const vs_attrs* attrs, const float* lo, const float* hi, const uint64_t* masks,
                   int64_t nq, int64_t* out, void* stream);
/* What vs_search would return over an index that held only the rows that pass
 * query q's predicate and are not in q's exclusion list (excl_offs /
 * excl_labels as vs_search_excl, NULL: none): vs_search's order, tie rules
 * (faiss's inner-product rule unless VS_RAW_ORDER), labels and padding;
 * exactly min(k, allowed matches) entries.  Any k.
 *
 * Route A (windows): the queries are searched in raw order for a window of w
 * entries (vs_distinct_plan's lengths), the entries whose row fails the
 * query's predicate are dropped, and a query whose window held fewer than it
 * needs and did not reach the end of the rows is searched again with a window
 * four times longer, while that is at most 1,023 entries or every live row.
 * Route B (the predicated scan): what is left is answered by the exact paged
 * kernels with the predicate and the exclusion list tested where a row enters
 * a query's list; batches of at most 32 queries stream the rows and skip the
 * 4-row steps no query wants.  A call of at most 32 queries counts its
 * predicates' rows first (vs_attrs_count's kernel) and sends a query whose
 * passing fraction is below 0.05 to route B at once; VS_WHERE_SCAN sends every
 * query there.  Route A returns the staged engine's keys (the fp32 rounding of
 * the exact score), route B the exact engines' fp32 keys, inside the
 * documented tolerance of those: a query's D bits may depend on the route.
 *
 * Checked before the index is read, in this order: the index, the handle,
 * n >= 0, k > 0 and k's bound (VS_E_INVALID); n == 0 is success; the bounds
 * (a NaN), the exclusion offsets, the buffers.  A handle of another index or
 * an older generation: VS_E_INVALID.  flags: VS_IN_DEVICE (x), VS_OUT_DEVICE
 * (D, I), VS_RAW_ORDER, VS_WHERE_SCAN.  The call reads a 4-byte count per
 * round, so it waits for `stream`; a capturing stream: VS_E_UNSUPPORTED. */
int vs_search_where(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const float* lo, const float* hi, const uint64_t* masks,
                    const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                    int flags, void* stream);
/* Diagnostic (touches no device): the windows of a where search for k over
 * `live` rows, round by round, then 0 for "the scan", or a last window equal
 * to `live` when no scan is needed: out[r] for r < nmax.  Returns the number
 * of entries of the whole plan (0 for live == 0), or VS_E_INVALID. */
int vs_where_plan(int64_t k, int metric, int raw, int64_t live, int64_t* out, int nmax);
/* Process-wide counters of the where searches since the last reset (reset != 0
 * clears them): queries searched, window rounds run (summed over the calls'
 * chunks), queries whose first window was too short, queries answered by the
 * scan, and the rows its streaming kernel loaded. */
int vs_where_stats(int64_t* searches, int64_t* rounds, int64_t* requeried, int64_t* scanned,
                   int64_t* rows_streamed, int reset);

/* ---- boosted searches ------------------------------------------------------
 * Exact top-k under similarity plus a per-query function of the row's
 * attributes (Qdrant's score boosting, Elasticsearch's function_score).  The
 * reference adds a reading-level match, a staff-pick bonus and further soft
 * terms to every candidate (src/recommendation_api/scoring.py:78-131), but only
 * to the k * 2 rows a plain similarity search returned; these calls rank every
 * row by the boosted score.
 *
 * For query q and live row r, with key the engine's key (-score for inner
 * product, the squared distance for L2):
 *   final_key(q, r) = fl32(key(q, r) - b(q, r))
 * and the result is the k rows with the smallest (final_key, label), in that
 * order (the lower label wins a tie, for both metrics).  D is -final_key
 * (= fl32(score + b)) for inner product and final_key for L2, where it may be
 * negative; padding is (-+FLT_MAX, -1).
 *
 * b(q, r) is float32, every operation rounded once to nearest, no FMA, the
 * division correctly rounded.  Column c of the handle contributes by
 * kinds[q][c] with params[q][c] = (t, s, w, miss) and the row's value v:
 *   0 none: +0
 *   1 near: w * max(0, 1 - |v - t| / s)
 *   2 ramp: w * min(1, max(0, (v - t) / s))
 * and `miss` when v is NaN and the kind is not 0 (max(0, x) is x > 0 ? x : +0,
 * min(1, y) is y < 1 ? y : 1).  Tag term j < 4 adds tag_bonus[q][j] when
 * (tags & tag_masks[q][j]) != 0, else +0.  b = (((c0 + c1) + c2) + c3) + g0 +
 * g1 + g2 + g3, left to right.  The same sum over max(0, w, miss) /
 * min(0, w, miss) of the columns whose kind is not 0 and max(0, bonus) /
 * min(0, bonus) gives the per-query bounds U >= b >= L.
 *
 * vs_search_boost (scoring.py:78-131's reading-level and staff-pick terms over
 * every row): kinds HOST int32 [n][ncol], params HOST [n][ncol][4] (ncol the
 * handle's; all finite, s > 0, else VS_E_INVALID), tag_masks / tag_bonus HOST
 * [n][4] or both NULL.  lo / hi / masks as vs_search_where (all NULL: no
 * predicate) and excl_offs / excl_labels as vs_search_excl compose with the
 * boost: a row that fails its predicate or is excluded is no candidate, the
 * others are ranked by the final key.  Any k.
 *
 * Route A (windows): the queries are searched in raw order for a window of w
 * entries (vs_where_plan's lengths for the raw order, at most 1,023), the
 * window is re-ranked by final key, and a query is settled when its window
 * reached the end of the rows or k entries were kept and final_key[k-1] <
 * fl32(K_w - U), K_w the window's last raw key: every row outside has a raw key
 * >= K_w and b <= U, so by monotone rounding a final key >= fl32(K_w - U).
 * An unsettled query is searched again with a window four times longer, or
 * sent to route B at once when its deficit exceeds the window's key spread.
 * Route B (the boosted scan): the exact paged kernels with the boost, the
 * predicate and the exclusion list applied where a row enters a query's list.
 * VS_BOOST_SCAN sends every query there.  As for vs_search_where, a query's D
 * bits may depend on the route, inside the engines' documented tolerance.
 *
 * Checked in vs_search_where's order: the index, the handle, n >= 0, k > 0 and
 * k's bound; n == 0 is success; the boost arrays, the bounds, the exclusion
 * offsets, the buffers.  A handle of another index or an older generation:
 * VS_E_INVALID.  flags: VS_IN_DEVICE (x), VS_OUT_DEVICE (D, I), VS_BOOST_SCAN.
 * The call reads a 4-byte count per round, so it waits for `stream`; a
 * capturing stream: VS_E_UNSUPPORTED. */
int vs_search_boost(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const int32_t* kinds, const float* params, const uint64_t* tag_masks,
                    const float* tag_bonus, const float* lo, const float* hi,
                    const uint64_t* masks, const int64_t* excl_offs, const int64_t* excl_labels,
                    float* D, int64_t* I, int flags, void* stream);
/* The definition of b on the host (scoring.py:78-131's soft terms as one
 * function; touches no device): cols HOST [ncol][nrows], tags HOST [nrows] or
 * NULL, the boost arrays of nq queries as above; b HOST [nq][nrows] =
 * b(q, r), bit for bit what the kernels compute, bounds HOST [nq][2] = L, U. */
int vs_boost_eval(int ncol, const float* cols, const uint64_t* tags, int64_t nrows,
                  const int32_t* kinds, const float* params, const uint64_t* tag_masks,
                  const float* tag_bonus, int64_t nq, float* b, float* bounds);
/* Process-wide counters of the boosted searches (the searches that replace
 * scoring.py:78-131's re-rank of k * 2 rows) since the last reset (reset != 0
 * clears them): queries searched, window rounds run (summed over the calls'
 * chunks), queries whose first window did not settle them, queries answered by
 * the scan. */
int vs_boost_stats(int64_t* searches, int64_t* rounds, int64_t* requeried, int64_t* scanned,
                   int reset);

/* ---- bonus searches ----------------------------------------------------------
 * Exact top-k under per-query, per-row score bonuses: the terms of the
 * reference's ranking formula that are numbers per (student, book) and not
 * functions of a book's attributes (scoring.py:116-125: the social term
 * gamma * neighbour_recent and the recency term), applied to every row instead
 * of to the k * 2 rows a plain search returned.
 *
 * Query q lists at most 1,024 pairs (label, s): bonus_offs HOST int64 [n + 1]
 * from 0, bonus_labels HOST [bonus_offs[n]], bonus_vals HOST float
 * [bonus_offs[n]].  Every s is finite and the labels of one list are distinct;
 * their order does not matter.  Labels that are not live labels of the index
 * (and -1) are ignored, as in vs_search_excl.  With key and b(q, r) as for
 * vs_search_boost (b = +0 when attrs is NULL),
 *   final_key = fl32(fl32(key - b) - s)   for a row q lists,
 *   final_key =      fl32(key - b)        otherwise,
 * two separately rounded subtractions, never contracted; a positive s improves
 * a row under both metrics and s = +0 changes nothing.  The result is the k
 * allowed rows (live, passing q's predicate, not in q's exclusion list) with
 * the smallest (final_key, label), the lower label first among equal keys
 * under both metrics; D is -final_key for inner product and final_key for L2,
 * padded with (-+FLT_MAX, -1).  A listed row that fails the predicate or is
 * excluded is no candidate, whatever its bonus.  Any k.
 *
 * attrs may be NULL: kinds, params, tag_masks, tag_bonus, lo, hi and masks must
 * then be NULL too (else VS_E_INVALID) and the base search is the plain search
 * in raw order (vs_search with VS_RAW_ORDER, vs_search_excl with lists).  With
 * a handle the arrays are exactly vs_search_boost's and the base search is
 * that call's (VS_BOOST_SCAN is passed through to it).  bonus_offs NULL or all
 * lists empty: the base search's answer bit for bit.
 *
 * Route: the base search ranks the allowed rows without the listed rows of
 * negative s (they join the query's exclusion segment; -0 counts as not
 * negative) by their bonus-free keys; every listed live row is scored directly;
 * the two sets are merged by (final_key, label).  An unlisted row of the true
 * top-k is in the base result, because every row that beats it in the
 * bonus-free order over that set also beats it in the final order (rounded
 * subtraction is monotone: fl32(x - s) <= x for s >= 0).  A listed row always
 * carries the rescoring's key (the fp64 sum rounded once, then the metric's
 * formula); an unlisted row carries the key of the base search's route, so, as
 * for vs_search_boost, a query's D bits may depend on the base route, inside
 * the engines' documented tolerance.
 *
 * Checked in vs_search_boost's order: the index, n >= 0, k > 0 and k's bound;
 * n == 0 is success; the boost arrays; the bonus lists (offsets that do not
 * start at 0 or decrease, a value that is not finite, a label twice in one
 * list: VS_E_INVALID; a list longer than 1,024: VS_E_UNSUPPORTED); the bounds,
 * the exclusion offsets, the buffers, the handle.  flags: VS_IN_DEVICE (x),
 * VS_OUT_DEVICE (D, I), VS_BOOST_SCAN.  The call waits for `stream`; a
 * capturing stream: VS_E_UNSUPPORTED. */
int vs_search_bonus(vs_index* idx, const vs_attrs* attrs, const float* x, int64_t n, int64_t k,
                    const int64_t* bonus_offs, const int64_t* bonus_labels,
                    const float* bonus_vals, const int32_t* kinds, const float* params,
                    const uint64_t* tag_masks, const float* tag_bonus, const float* lo,
                    const float* hi, const uint64_t* masks, const int64_t* excl_offs,
                    const int64_t* excl_labels, float* D, int64_t* I, int flags, void* stream);
/* Process-wide counters of the bonus searches since the last reset (reset != 0
 * clears them): queries searched, listed live rows scored, queries whose base
 * search carried at least one extra exclusion (a listed live row of negative
 * s), result entries that are listed rows.  With a handle the base searches
 * count in vs_boost_stats as well. */
int vs_bonus_stats(int64_t* searches, int64_t* listed, int64_t* demoted, int64_t* entered,
                   int reset);

/* ---- example searches ------------------------------------------------------
 * Recommendation from examples (Qdrant recommend, strategy="best_score"): the
 * rows nearest to ANY liked example that no disliked example is at least as
 * near to.  The reference's reader path (src/recommendation_api/service.py:
 * 423-554) averages the rated books into one query, where a thumbs-down only
 * shrinks a weight (the disliked book still pulls the query towards itself)
 * and two tastes average into a query near neither; vs_search_profiles keeps
 * that mean bit for bit, these calls use the examples themselves.
 *
 * The index metric decides the key as everywhere: key = distance (L2) or
 * -score (inner product), smaller is better.  key(e, r) of an example vector e
 * and a stored row r is the rescoring's exact key: the fp64 sum of the
 * products rounded once to fp32, then L2: max(0, (|e|^2 + |x|^2) - 2 e.x) with
 * the staged |e|^2 and the stored |x|^2 — always this form, however many
 * examples the call holds, so a user's answer does not depend on who else is
 * in the call — or inner product: -e.x.  bf16 indexes round the example to
 * bf16 first, as searches round their queries.
 *
 * For user u with positives P (at least one), negatives N (possibly none) and
 * allowed rows A = the live rows minus u's exclusion list:
 *   p(r) = min over e in P of key(e, r); the deciding example of r attains it,
 *          among equal keys the lowest position in u's positive list;
 *   n(r) = min over e in N of key(e, r), +inf without negatives;
 *   r is favoured iff p(r) < n(r) — strictly: a row exactly as near to a
 *   disliked example as to a liked one is not recommended.
 * The result is the first k favoured rows of A in ascending (p, label) order
 * (VS_RAW_ORDER's order; faiss's inner-product tie rule is not applied): this
 * is Qdrant's best_score order cut where its score changes sign.  Fewer than k
 * favoured rows pad with (+FLT_MAX | -FLT_MAX, -1).  D = p as a score (the
 * distance, or the inner product), I = the label, E (n * k int32, may be NULL)
 * = the deciding positive's position in the user's list, -1 on padding: the
 * "because you liked X" of a recommender.
 *
 * vs_search_examples: the examples are stored rows by label, HOST CSRs as
 * vs_mean_rows takes them (pos_offs / neg_offs: n + 1 int64 from 0; neg_offs
 * may be NULL).  A label that is not a live label: VS_E_INVALID.  excl_offs /
 * excl_labels as vs_search_excl (NULL: none); exclude_examples != 0 adds every
 * example label of a user to that user's exclusion list.
 * vs_search_examples_x: the same search with the examples as fp32 vectors,
 * pos_x = pos_offs[n] * d and neg_x = neg_offs[n] * d floats in CSR order
 * (VS_IN_DEVICE covers these two arrays).  Both forms converge on one device
 * matrix of example rows — labels are gathered from the index (bf16 widened,
 * as vs_reconstruct_n returns them), vectors are staged as queries are — so
 * with stored rows given either way they return the same bits.
 * flags: VS_OUT_DEVICE covers D, I and E.
 *
 * Exact (DESIGN.md "Example searches"): a round searches every positive of the
 * users still unsettled in raw order for a window of w entries (the distinct
 * searches' schedule: k + max(16, k / 2), four times longer every round, at
 * last every live row), each positive with its user's exclusion list.  With F
 * the smallest last entry of a user's windows, the rows at or before F in
 * (p, label) order are known exactly; if k of them are favoured, or every
 * window reached the end of the allowed rows, the user is settled, otherwise
 * it alone is searched again.  The members of that set are rescored with the
 * exact key before they are compared with the negatives and ordered (the same
 * bits where the engine's key is the exact key already, as on fp32 indexes; a
 * bf16 index's large batches accumulate in fp32, and there only the windows
 * keep that engine's order).  A user with fewer than k favoured rows pays for
 * the long windows: past 1,023 entries the paged engine answers, about w / 64
 * passes over the rows per positive.  A round's scratch is 72 bytes per window
 * entry, in batches of users of at most 1 GiB; a user whose own windows
 * (positives x w) exceed that: VS_E_UNSUPPORTED when that round is reached.
 *
 * Checked before the index is read, in this order: the index, n >= 0, k > 0
 * (VS_E_INVALID); k > 1024: VS_E_UNSUPPORTED; the offsets start at 0 and do
 * not decrease; every user has at least one positive (VS_E_INVALID); more than
 * 64 positives or 64 negatives of one user: VS_E_UNSUPPORTED (the reference
 * caps a reader's history at 20 books, config.py:24); the exclusion offsets;
 * the buffers.  n == 0 is success.  The call reads a 4-byte count after every
 * round, so it waits for `stream`; a capturing stream: VS_E_UNSUPPORTED.
 * Every user's examples lie in one engine chunk (65,536 positives). */
int vs_search_examples(vs_index* idx, const int64_t* pos_offs, const int64_t* pos_labels,
                       const int64_t* neg_offs, const int64_t* neg_labels, int64_t n, int64_t k,
                       const int64_t* excl_offs, const int64_t* excl_labels, int exclude_examples,
                       float* D, int64_t* I, int32_t* E, int flags, void* stream);
int vs_search_examples_x(vs_index* idx, const int64_t* pos_offs, const float* pos_x,
                         const int64_t* neg_offs, const float* neg_x, int64_t n, int64_t k,
                         const int64_t* excl_offs, const int64_t* excl_labels, float* D, int64_t* I,
                         int32_t* E, int flags, void* stream);
/* Process-wide counters of the example searches since the last reset
 * (reset != 0 clears them): users searched, rounds run (summed over the calls'
 * chunks of users), and users whose first windows were too short (searched
 * again at least once). */
int vs_examples_stats(int64_t* users, int64_t* rounds, int64_t* requeried, int reset);

/* ---- MMR searches ----------------------------------------------------------
 * LangChain's maximal-marginal-relevance searches
 * (FAISS.max_marginal_relevance_search*, as_retriever(search_type="mmr")):
 * search fetch_k rows, then pick k of them greedily, each pick trading its
 * similarity to the query against its similarity to the picks before it.  The
 * reference appends a second row when a book is re-ingested
 * (src/incremental_workers/book_vector/main.py:148), so a plain top-k can
 * return one book twice, and its cooldown logic exists "to improve
 * recommendation diversity" (src/recommendation_api/service.py:1104, 1398).
 * LangChain re-ranks on the host (reconstruct every candidate, numpy cosine
 * matrices, a Python loop per query); here the candidates stay in HBM.
 *
 * The definition is langchain_community.vectorstores.utils
 * maximal_marginal_relevance / cosine_similarity (0.3.x) as recalled:
 * langchain is not vendored.  For one query q and its candidate list
 * c_0 .. c_{F-1} (stored rows by label; -1 is an empty slot, no candidate, but
 * it keeps its position):
 *   cos(a, b) = dot(a, b) / sqrt(dot(a, a) * dot(b, b)), every dot product a
 *   sum in fp64 of the exact products of the fp32 values (bf16 indexes: the
 *   stored value widened to fp32, as vs_reconstruct_n returns it; the query is
 *   never rounded); a non-finite quotient (a zero-norm row or query) counts as 0.
 *   With s_i = cos(q, c_i): the first pick is the candidate with the largest
 *   s_i; each later pick maximises
 *     lambda_mult * s_i - (1 - lambda_mult) * max_{j picked} cos(c_i, c_j)
 *   over the candidates not yet picked, evaluated in fp64; ties go to the
 *   lowest position (LangChain compares with strict > in list order); the
 *   selection stops after min(k, candidates) picks.
 * The summation order inside a dot product is the kernel's own but fixed (no
 * atomics, no dependence on a candidate's position or on the batch): results
 * are bit-identical from run to run and equal rows get equal scores.  Not
 * promised: which of two candidates wins when their scores differ by less
 * than the rounding of those sums, (4d + 16) * 2^-53.
 *
 * Both calls check, before the index is read and in this order: the index,
 * n >= 0, k > 0, fetch_k > 0, lambda_mult finite, the buffers (VS_E_INVALID);
 * fetch_k > 1024 is VS_E_UNSUPPORTED (the staged engine's candidate limit;
 * callers re-rank longer lists in pieces).  k > fetch_k is legal, n == 0 is
 * success.  The re-rank's scratch stays within 64 MiB per chunk of queries.
 *
 * vs_mmr_select: the positions (into each query's candidate list) chosen by
 * MMR, in pick order.  cand: n * fetch_k int64 labels (id_base applied as
 * everywhere), -1 allowed anywhere, a duplicate label simply a duplicate
 * candidate; any other label that is not a live label: VS_E_INVALID (faiss
 * reconstruct throws).  pos: n * k int32, -1 past min(k, candidates).
 * VS_IN_DEVICE covers x and cand (the call then waits for `stream` to read
 * one validity flag), VS_OUT_DEVICE covers pos. */
int vs_mmr_select(vs_index* idx, const float* x, int64_t n, const int64_t* cand, int64_t fetch_k,
                  int64_t k, double lambda_mult, int32_t* pos, int flags, void* stream);
/* vs_search / vs_search_excl for fetch_k, then the selection: D, I = the chosen
 * entries' faiss scores and labels in pick order, padded (+-FLT_MAX, -1).  The
 * candidate order is exactly what vs_search / vs_search_excl return for
 * k = fetch_k (inner product: faiss's tie order); fetch_k past the live rows
 * pads, and the padding slots are empty slots.  excl_offs / excl_labels as
 * vs_search_excl (NULL: none).  VS_IN_DEVICE applies to x, VS_OUT_DEVICE to D
 * and I; the stream contract is vs_search_excl's.  The candidates never leave
 * the device (n * fetch_k scores and labels of scratch, as a search with
 * device outputs holds).  Callers: FAISS.max_marginal_relevance_search*. */
int vs_search_mmr(vs_index* idx, const float* x, int64_t n, int64_t k, int64_t fetch_k,
                  double lambda_mult, const int64_t* excl_offs, const int64_t* excl_labels,
                  float* D, int64_t* I, int flags, void* stream);

/* ---- range search ----------------------------------------------------------
 * faiss IndexFlat::range_search(n, x, radius, result[, params.sel]): every row
 * within the radius, as many as there are — strict comparisons as faiss, L2:
 * squared distance < radius, inner product: score > radius.  Replaces the
 * reference's thresholds applied after a k-bounded search
 * (src/graph_refresher/main.py:339-354 similarity_threshold,
 * src/recommendation_api/mcp_book_server.py:818-896 min_similarity, LangChain's
 * score_threshold), which cut "everything at least this similar" at a guessed k.
 *
 * A row is decided by its EXACT key alone (fp64 sum rounded once, the key the
 * staged engine's rescoring returns: L2 calls with n < 20 as the direct sum of
 * squares, n >= 20 as |q|^2 + |x|^2 - 2 q.x clamped at 0; bf16 indexes over the
 * stored values and bf16-rounded queries), so the result does not depend on
 * tiling or batch padding and is bit-identical from run to run.  D holds that
 * key as a score (distance / inner product).  Each query's hits come in
 * ascending label order.  A NaN radius and rows with NaN keys (tombstoned rows)
 * match nothing.  A non-NULL selector restricts the hits to its rows (a stale
 * one: VS_E_INVALID, as vs_search_sel).
 *
 * The result handle owns device buffers and outlives the index.  The call
 * always synchronises `stream` (it reads two totals to size its buffers; on a
 * capturing stream: VS_E_UNSUPPORTED).  n == 0 or an empty index: success, lims
 * all 0.  n > 65536, or 2^31 or more candidates or hits: VS_E_UNSUPPORTED
 * (callers chunk the queries).  flags: VS_IN_DEVICE. */
typedef struct vs_range vs_range;
int vs_range_search(vs_index* idx, const vs_selector* sel /* may be NULL */, const float* x,
                    int64_t n, float radius, int flags, void* stream, vs_range** out);
int vs_range_size(const vs_range* r, int64_t* nq, int64_t* total);
/* The rows the candidate passes handed to the verification (>= total; the
 * difference is the price of the preselection's bound).  Library-specific;
 * tools/bench_range.py reports it. */
int vs_range_candidates(const vs_range* r, int64_t* out);
/* lims: nq + 1 int64 (lims[0] = 0, lims[nq] = total); D / I: total entries
 * (query q's hits are [lims[q], lims[q + 1])).  VS_OUT_DEVICE: all three are
 * device pointers on the index's device, the copy stream-ordered on `stream`. */
int vs_range_copy(const vs_range* r, int64_t* lims, float* D, int64_t* I, int flags, void* stream);
int vs_range_destroy(vs_range* r);

/* faiss Index::reconstruct_n(i0, n, out) / reconstruct(i) — rows as added
 * (bf16 storage returns the stored bf16 value widened to float32).
 * Callers: store.index.reconstruct at candidate_builder.py:166-168, service.py:490-494. */
int vs_reconstruct_n(vs_index* idx, int64_t i0, int64_t n, float* out, int flags, void* stream);

/* faiss IndexFlat::remove_ids(IDSelectorBatch(ids)) — stable compaction; ids
 * outside [0,ntotal) and duplicates are ignored; *nremoved = rows removed.
 * Caller: langchain FAISS.delete (BASELINE config 5 add/remove). */
int vs_remove_ids(vs_index* idx, const int64_t* ids, int64_t n, int64_t* nremoved);

/* Cosine self-join — replaces the per-student pgvector query
 *   SELECT student_id, 1-(vec <=> src.vec) ... WHERE student_id <> $1
 *   ORDER BY vec <=> src.vec LIMIT 15
 * at src/graph_refresher/main.py:339-354 and src/incremental_workers/similarity/main.py:80-87.
 * For stored rows q in [q0, q0+nq): the k rows with largest cosine similarity
 * dot/sqrt(|a|^2 |b|^2) (ties: lower row first; any k, as SQL's LIMIT), excluding row q itself when
 * exclude_self != 0.  Entries whose similarity is < min_sim (the
 * graph_refresher's S.similarity_threshold filter, main.py:350-354) are returned
 * as (-FLT_MAX, -1).  Zero-norm rows never match (pgvector yields NaN for them).
 * D is nq*k similarities, I is nq*k labels (id_base applied). */
int vs_selfjoin(vs_index* idx, int64_t q0, int64_t nq, int64_t k, int exclude_self,
                float min_sim, float* D, int64_t* I, int flags, void* stream);

/* Range self-join: the student graph without its LIMIT.  For stored rows q in
 * [q0, q0+nq): EVERY row r whose cosine similarity with row q is >= min_sim, as
 * many as there are — the edges `sim >= S.similarity_threshold` that
 * src/graph_refresher/main.py:339-354 keeps and that its `LIMIT 15` (SQL needs
 * a k; also src/incremental_workers/similarity/main.py:80-94) cuts at the 15th
 * neighbour in a dense cluster.  The comparison is not strict (vs_selfjoin's
 * min_sim, the reference's sim >= threshold).
 *
 * A pair is decided by its exact key alone: the fp64 sum of the two stored
 * rows' products (fp32 x fp32, or bf16 x bf16) rounded once, times the product
 * of the two rows' inverse norms.  That key is the same bits for (a, b) and
 * (b, a), so the full join is symmetric, and `upper` != 0 — a query row
 * reports only the rows after it, r > q — is exactly that half of it, found
 * with half the multiplications (row tiles below the diagonal are skipped).
 * exclude_self != 0 leaves row q out of its own hits; `upper` leaves it out by
 * itself.  Zero-norm rows and a NaN min_sim match nothing.
 *
 * The result is a vs_range handle (vs_range_size / vs_range_copy /
 * vs_range_destroy): D holds the similarities, I the labels row + id_base, each
 * query's hits in ascending row order.  q0 is a row position; an index with
 * tombstones is packed first (as vs_selfjoin).  The call synchronises `stream`
 * (a capturing stream: VS_E_UNSUPPORTED).  nq == 0 or an empty index: lims all
 * 0.  nq > 65536, or 2^31 or more candidates: VS_E_UNSUPPORTED (callers chunk
 * the query rows).  flags: none yet (pass 0). */
int vs_range_selfjoin(vs_index* idx, int64_t q0, int64_t nq, float min_sim, int exclude_self,
                      int upper, int flags, void* stream, vs_range** out);

/* vs_range_selfjoin with the query rows given as a list: qrows is HOST int64,
 * nq row positions in any order, duplicates allowed; entry i gets segment i of
 * lims.  The exact key, the not-strict comparison, the zero-norm rule, the
 * pack of tombstones first, the 65536-row and 2^31 limits, the refusal of a
 * capturing stream and the result handle are vs_range_selfjoin's: a segment is
 * bit-identical to the one vs_range_selfjoin(q0 = row, nq = 1) returns, and
 * symmetry holds.  A position outside [0, ntotal), checked after the pack, is
 * VS_E_INVALID.  There is no `upper` (the triangle needs a window).  One pass
 * over the rows serves 128 listed rows: the edges of a batch of re-embedded
 * students (vs_update_rows) are its complete diff of the graph. */
int vs_range_selfjoin_rows(vs_index* idx, const int64_t* qrows, int64_t nq, float min_sim,
                           int exclude_self, int flags, void* stream, vs_range** out);

/* Merge nparts per-shard top-k lists into one (faiss: the ResultHandler merge;
 * GPU-side half of the RCCL all-gather top-k merge).  Inputs are DEVICE arrays
 * laid out [nparts][nq][k_in] (scores + int64 labels, -1 = empty; raw order for
 * inner product, any k_in and k, nparts <= 64); outputs are DEVICE arrays
 * [nq][k].  metric picks the order (L2 ascending, IP descending). */
int vs_merge_topk(const float* D_parts, const int64_t* I_parts, int64_t nparts, int64_t nq,
                  int64_t k_in, int64_t k, int metric, float* D, int64_t* I, void* stream);

/* Writes rows x[i][j] = ((splitmix64(seed ^ ((row0+i)*d + j)) >> 40) * 2^-23) - 1
 * (exactly representable float32 in [-1,1)) into a DEVICE buffer of rows*d floats.
 * The same generator is restated in python for the oracle (vsearch.synth). */
int vs_fill_synthetic(float* out, int64_t rows, int64_t d, uint64_t seed, int64_t row0,
                      void* stream);

/* ---- measurement ----------------------------------------------------------
 * When enabled, every launch of the dominant search kernel (the fused
 * distance+top-k kernel) is bracketed by HIP events on the launch stream.
 * vs_timer_read synchronises those events and returns the summed kernel time in
 * milliseconds and the number of kernel dispatches inside the timed spans since
 * the last reset (gemm_topk_x1 cuts one search into several dispatches). */
int vs_timer_enable(int on);
/* Queries searched by the filter-and-verify engine and how many of them the
 * exact engine had to redo, since the last reset (reset != 0 clears them). */
int vs_filter_stats(int64_t* queries, int64_t* fallbacks, int reset);
/* Of those queries, how many the first check flagged and the wide check (every
 * lane-list entry below the list floors rescored) examined again, since the last
 * vs_filter_stats reset.  Diagnostic only: no reference interface. */
int vs_filter_wide_stats(int64_t* wide);
/* Queries the staged engine handed from the int8 plane to the bf16 plane since
 * the last vs_filter_stats reset.  Diagnostic only: no reference interface. */
int vs_filter_second_stats(int64_t* second);
/* Queries the staged engine's last stage could not prove from its fp32 GEMM
 * candidates (dense near-ties inside the fp32 bound) and ranked over every row
 * by the exact key instead (vs_exact.hip), since the last vs_filter_stats
 * reset.  Diagnostic only: no reference interface. */
int vs_filter_exact_stats(int64_t* streamed);
/* Entries the wide checks examined (summed over queries) and how many of them
 * were read from HBM and rescored (the rest reuse the first check's exact keys),
 * since the last vs_filter_stats reset.  Diagnostic only: no reference interface. */
int vs_filter_wide_sets(int64_t* entries, int64_t* rescored);
/* Rows the filter pass's dump launches stored (one (row, raw sum) slot per
 * row that may lie below its lane list's floor) and lane lists that ran out of
 * dump slots
 * (their queries went to the next stage), since the last vs_filter_stats
 * reset.  Diagnostic only: no reference interface. */
int vs_filter_dump_stats(int64_t* dumps, int64_t* overflows);
int vs_timer_reset(void);
/* Diagnostic only (no reference interface): the filter pass's per-segment
 * cycle sums of a stamp build (VS_X1_STAMP=1; zeros otherwise), 58 values:
 * [waves 0-3 | 4-7][load issue, vmcnt wait, barrier 1, matrix issue,
 * barrier 2, epilogue, epilogue reject, factor loads, keys and inserts;
 * factor-load paths, inserting blocks, inserts]
 * then the steps of each group, then the 16x16x64 dump launches' events per
 * lane and launch as two histograms of 0 .. 15+ (the pass's first dump launch,
 * the later ones); reset != 0 clears them. */
int vs_x1_stamps(unsigned long long* out, int reset);
/* Diagnostic only (no reference interface; touches no device): the launches
 * of one filter pass over ntotal rows in nsplit workgroup splits, as the
 * library would run it under the environment's VS_X1_* knobs.  mode: the
 * kernel mode (0 inner product, 1 L2, 2 cosine); filter: 0 the bf16 plane,
 * 1 int8; can_dump: the search gave the pass dump buffers and cuts; ecut: its
 * cuts are also exact-key cuts; gathered: a later stage's gathered batch;
 * recut: 0 one cut per pass, 1 or 2 a new cut after every replay but the last.
 * out holds 5 + 4 cap values:
 *   out[0] parts the pass cuts every workgroup's tiles into, out[1] the first
 *   launch's lists set cuts, out[2] always 0 (it marked a launch form that was
 *   removed; kept so the other values keep their indices), out[3] the
 *   launches after the first are dump launches, out[4] the same question as
 *   the search asks it before allocating dump buffers (from ntotal and nsplit
 *   alone: equal to out[3] of the call with can_dump = 1, gathered = 0);
 *   then {p0, p1, kind, after} per launch, the first min(cap, *nlaunch):
 *   parts [p0, p1); kind 0 list, 2 dump on 32x32x32 MFMAs, 3 dump on
 *   16x16x64 (1, the removed form, is never produced); after, a mask of what runs next in this order: 1 replay,
 *   2 the first cut, 4 replay and a new cut, 8 an exact-key cut.
 * *nlaunch = the pass's launches. */
int vs_x1_plan(int mode, int filter, int64_t ntotal, int nsplit, int can_dump, int ecut,
               int gathered, int recut, int32_t* out, int cap, int* nlaunch);
int vs_timer_read(double* total_ms, int64_t* launches);
/* The same for the spans of one kernel name only (the filter engine's first
 * stage is "gemm_topk_x1_i8" or "gemm_topk_x1" (bf16) per search; its first
 * launch, when the later ones dump, "<name>_list"; the whole pass including
 * the cut and replay kernels "<name>_pass", a span that vs_timer_read's total
 * leaves out because its kernels are in the other spans). */
int vs_timer_read_kernel(const char* kernel, double* total_ms, int64_t* launches);
/* The same, plus the summed share of their passes' database tiles that those
 * spans covered (a filter pass's launches cover unequal parts: its list
 * launch a quarter chunk or 1/8 of a split pass; bench.py's roofline work). */
int vs_timer_read_kernel_share(const char* kernel, double* total_ms, int64_t* launches,
                               double* share);
/* Name of the fused search kernel the last search launched ("gemm_topk_x1",
 * "gemm_topk", "skinny_topk" or "gemv_topk"). */
const char* vs_timer_kernel(void);

#ifdef __cplusplus
}
#endif

#endif /* VSEARCH_H */
