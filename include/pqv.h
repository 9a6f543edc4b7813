/*
 * pqv.h -- C ABI of the MI355X-native pq-vector hot path (libpqv_hip.so).
 *
 * This is the drop-in boundary.  The reference (pure Rust, no FFI of its own) would bind
 * these symbols from a `extern "C"` block where its L1 "IVF core" meets its callers; each
 * entry point cites the reference interface it replaces (paths relative to the reference
 * repo).  INTEGRATION.md shows the Rust-side binding.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types.
 *   - return 0 (PQV_OK) or a negative pqv_status; the message for the calling thread is
 *     returned by pqv_last_error().  Validation messages are the reference's own strings
 *     (src/ivf/index.rs:24,89,158,169; src/ivf/mod.rs:59,86; src/ivf/parquet.rs:90,93;
 *     src/ivf/search.rs:67,72,92-97) so a Rust shim can surface identical errors.
 *   - inputs are borrowed for the duration of the call (mirrors `&[f32]`); outputs are
 *     either caller-allocated fixed-size arrays or library buffers released with the
 *     matching pqv_*_free.  Opaque handles own host + device memory.
 *   - every entry point is blocking and callable from any thread.  A handle may be shared
 *     across threads; calls on one pqv_searcher serialise on its internal scratch.
 *   - there is NO CPU fallback: every compute entry point fails with PQV_ERR_NO_DEVICE
 *     when no gfx950 device is usable.
 *   - row ids are file-global u32 row ordinals, as in the reference (src/ivf/index.rs:13).
 */
#ifndef PQV_H
#define PQV_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum pqv_status {
    PQV_OK              = 0,
    PQV_ERR_INVALID     = -1,  /* argument validation (reference's message texts)      */
    PQV_ERR_NO_DEVICE   = -2,  /* no usable HIP device / device index out of range      */
    PQV_ERR_HIP         = -3,  /* a HIP runtime call failed                              */
    PQV_ERR_OOM         = -4,  /* host or device allocation failed                       */
    PQV_ERR_UNSUPPORTED = -5,  /* outside the implemented envelope (e.g. k > 1024)       */
    PQV_ERR_FORMAT      = -6   /* malformed index blob                                   */
} pqv_status;

/* Summation order of the squared-L2 distance. */
typedef enum pqv_metric {
    PQV_L2SQ_REF4 = 0, /* src/ivf/index.rs:461-480: sum += ((d0^2+d1^2)+d2^2)+d3^2 per 4 */
    PQV_L2SQ_SEQ  = 1  /* src/df_vector/exec.rs:529-533: dist += d^2, element by element */
} pqv_metric;

/* Metrics of pqv_brute_topk (an EXTENSION: the reference has neither cosine distance nor a
 * batched brute-force path -- SURVEY F5; BASELINE.json configs[4] asks for it).  Every returned
 * distance comes from an f32 dot product (f32 matrix cores for the first rows, an exact f32
 * re-scoring behind the int8 / f16 matrix-core screen of the rest: the screen is a rigorous
 * bound, it never drops a row of the result), so distances agree with an f64 oracle to ~1e-6
 * relative (well inside the north star's 1e-4), not bit for bit.  The first call builds the
 * screen's image of the corpus (+ 1 byte per value; PQV_BRUTE_OP=f16: + 2). */
#define PQV_COSINE      2   /* 1 - q.v / (|q| |v|); zero-norm vectors get distance 1            */
#define PQV_L2SQ_MFMA   3   /* |q|^2 + |v|^2 - 2 q.v (norm-expansion form, clamped at 0)        */
/* PQV_COSINE through the index (pqv_topk, pqv_topk_device(_flags), pqv_range_search, pqv_searcher_describe, plain and table
 * searchers; an EXTENSION like the above, with arithmetic of its own).  With
 *   sq(v) = the PQV_L2SQ_REF4 chain of v against 0 (index.rs:461-480: 4-grouped, the tail element by element),
 *   r(v)  = 1.0f / sqrtf(sq(v)) (correctly rounded sqrt and division), 0 where sq(v) == 0,
 *   n(v)  = v_i * r(v) (one f32 multiply per value),
 * a cosine call returns exactly what the same call with PQV_L2SQ_REF4 and sqrt_out = 0 returns on a searcher over
 * Index.from_parts(dim, n(centroids) row by row, the same lists) and a corpus of n(x) for every row x, with the queries replaced by
 * n(q) -- row ids, n_found, n_candidates, counters, the tie rules (pqv_topk replays the heap on tied d2, pqv_topk_device orders by
 * (d2, position)), max_candidates (a table's round-robin cap too), a table's per-file nprobe, the device entry points' limits and the
 * range order included -- except that every distance is the f32 product 0.5f * d2: half the squared distance of the unit vectors,
 * 1 - cos(q, x) in exact arithmetic without the cancellation of 1 - q.x / (|q||x|) near 0.  So the probe ranks centroids by cosine
 * (ties by centroid id) and scaling q by a power of two changes no bit.  sqrt_out is ignored (the output is always this distance);
 * pqv_range_search's hit test is 0.5f * d2 <= radius.  ZERO vectors: a zero row or centroid normalises to 0 (distance
 * 0.5 * sq(n(q)) from a query), a zero query to 0 (every row at 0.5 * sq(n(x))) -- unlike pqv_brute_topk, which gives them 1.
 * The first cosine call on a searcher (or PQV_PREPARE_COSINE at creation) builds its cosine layout under the searcher's lock,
 * synchronously: the normalised centroid table and rows (one more f32 copy of the column, counted by pqv_searcher_footprint) and
 * the screen operands made from them; until then no L2 call or buffer is touched.  A failed build (PQV_ERR_OOM, ...) leaves the
 * searcher as it was.  Cosine queries are normalised on the device (one extra launch on the call's stream; pqv_topk_device stays
 * asynchronous after the first call); the halving is part of the final write-out.  pqv_rerank* and PQV_L2SQ_MFMA stay as they are:
 * no cosine through the index for the first, brute force only for the second. */
#define PQV_DOT         4   /* inner product: dist = -(q.x), the negated similarity (pgvector's <#>)  */
/* PQV_DOT through the index (pqv_topk, pqv_topk_device(_flags), pqv_range_search, the three masked forms, pqv_searcher_describe,
 * plain and table searchers; an EXTENSION like cosine: the reference has no inner product).  All operations are f32, each rounded
 * on its own:
 *   s(q, x):  sum = 0.0f
 *             per full group of four dims:  t = q0*x0 + q1*x1;  t = t + q2*x2;  t = t + q3*x3;  sum = sum + t
 *             tail (dim % 4 values), element by element:  sum = sum + qe*xe
 *   dist(q, x) = 0.0f - sum      (a zero result is always +0.0f, never -0.0f)
 * -- index.rs:461-480's grouping with products in place of squared differences, so s(x, x) is bit-equal to the PQV_L2SQ_REF4 chain
 * of x against 0.  Candidates are ordered by (dist, candidate position); NaN distances follow the order of
 * ord(b) = b ^ (b >> 31 ? 0xFFFFFFFF : 0x80000000) on their f32 bits and are unpinned, as everywhere.
 * A PQV_DOT call behaves as the PQV_L2SQ_REF4 call of the same arguments, except:
 *   probe        centroids are ranked ascending by (dist(q, centroid), centroid id), the first min(nprobe, n_clusters) are probed; a
 *                table searcher does so per file.  The candidate order, positions, max_candidates, a table's round-robin quotas
 *                and n_candidates follow from that probe, unchanged.  pqv_probe and pqv_candidate_rows take no metric: L2.
 *   result       the k candidates with the smallest (dist, position), ascending.  There is no reference heap to replay: pqv_topk
 *                and pqv_topk_device return the same thing, exact_replays never advances and d_tie_flags (where given) is written
 *                with zeros.  Entries past n_found[q] are 0xFFFFFFFF / +inf.  sqrt_out is ignored.
 *   range        a hit iff dist <= radius, any non-NaN radius: a negative one is ordinary (radius = -0.8 keeps s >= 0.8), +inf
 *                keeps every non-NaN candidate.  Order, max_results, n_within and the CSR output are unchanged.
 *   masks        pqv_topk_masked, pqv_topk_masked_device and pqv_range_search_masked take PQV_DOT under the masked contract as
 *                written (cap before mask, unmasked positions, excluded rows never read): bit-equal to the unmasked DOT call
 *                over pqv_index_from_parts(dim, centroids, [each list's allowed rows]), n_candidates excepted.
 *   path         always the exact stream per (query, probed list) over the centroids and the f32 rows in place, in every layout;
 *                no searcher option changes a DOT result and no layout is built lazily.
 *   limits       k <= 1024 (1023 with tie flags) and at most 1024 probed lists per query for EVERY DOT entry point, host and
 *                range forms included: beyond that PQV_ERR_UNSUPPORTED "PQV_DOT takes k <= 1024 and at most 1024 probed lists
 *                per query".
 *   counters     queries, candidate_rows and embeddings_fetched advance as for the L2 (masked L2) call of the same shape;
 *                screened_pairs and screen_survivors do not advance.
 * pqv_topk_keyed*, pqv_range_search_keyed and pqv_topk_distinct* with PQV_DOT return PQV_ERR_UNSUPPORTED "PQV_DOT is not supported
 * by keyed and distinct calls"; pqv_rerank* and pqv_brute_topk keep their metric checks. */

/* pqv_searcher_create flags */
#define PQV_LAYOUT_IVF_ORDERED   0x0u /* copy rows into cluster-contiguous order in HBM (default) */
#define PQV_LAYOUT_ROW_ORDER     0x1u /* keep file row order; re-rank gathers rows by id          */
#define PQV_RELEASE_ROW_ORDER    0x2u /* with IVF_ORDERED: let the corpus drop its row-order copy */
#define PQV_RELEASE_IF_COPIED    0x4u /* with IVF_ORDERED: drop the row-order copy only where the searcher made a list-ordered
                                         f32 copy of its own (the images-only layout keeps reading the caller's rows): one f32
                                         copy of the column resident either way                                              */
#define PQV_TABLE_CAP_ROUND_ROBIN 0x8u /* pqv_table_searcher_create: max_candidates is dealt out round robin over the files
                                          (see there); ignored by pqv_searcher_create                                         */
#define PQV_PREPARE_COSINE      0x10u  /* build the PQV_COSINE layout at creation (see PQV_COSINE), so that no query pays for it; the
                                          searcher is not returned when that fails                                             */

typedef struct pqv_index    pqv_index;    /* IvfIndex: dim, n_clusters, centroids, inverted lists */
typedef struct pqv_corpus   pqv_corpus;   /* the embedding column, resident in one GPU's HBM     */
typedef struct pqv_searcher pqv_searcher; /* (index, corpus) bound for querying on one GPU       */

/* Thread-local message of the last failing call on this thread ("" if none). */
const char *pqv_last_error(void);
/* Number of usable HIP devices (0 on a machine without a GPU; never an error). */
int pqv_device_count(void);
/* Library ABI version (major*100 + minor). */
int pqv_abi_version(void);

/* ---- embedding column -> HBM ---------------------------------------------------------
 * Replaces the materialised `Embeddings{data: Vec<f32>, dim}` that
 * read_parquet_with_embeddings hands to build_ivf_index (src/ivf/parquet.rs:216-305,
 * src/ivf/mod.rs:72-102) and the per-query read_embeddings_for_rows gather
 * (src/ivf/search.rs:155-244): the column is uploaded once and stays resident. */

/* rows: host [n, dim] row-major f32.  n may be 0 (build then fails like the reference). */
int pqv_corpus_upload(int device, const float *rows, uint64_t n, uint32_t dim,
                      pqv_corpus **out);
/* Append-style upload for streaming row groups: create empty with capacity, then append. */
int pqv_corpus_create(int device, uint64_t capacity_rows, uint32_t dim, pqv_corpus **out);
int pqv_corpus_append(pqv_corpus *corpus, const float *rows, uint64_t n_rows);
/* Same, narrowing a Float64 column to f32 first (src/ivf/parquet.rs:246-256). */
int pqv_corpus_append_f64(pqv_corpus *corpus, const double *rows, uint64_t n_rows);
/* Streaming upload for a loader that decodes row groups on several threads (N1; src/ivf/parquet.rs:216-305 materialises the
 * column batch by batch, :262-286): rows [row_offset, row_offset + n_rows) of a corpus made by pqv_corpus_create are written from
 * `rows`.  The call copies them into one of the corpus' PINNED staging buffers and enqueues the DMA (hipMemcpyAsync); it returns
 * as soon as the caller's buffer may be reused, so decoding the next batch overlaps the upload of this one.  Batches may arrive
 * in any order and from several threads.  _f64 narrows `as f32` on the device (:246-256).  pqv_corpus_finish waits for every
 * DMA and sets the row count to n_rows (<= capacity); until then the corpus must not be used by anything else. */
int pqv_corpus_write_rows(pqv_corpus *corpus, uint64_t row_offset, const float *rows, uint64_t n_rows);
int pqv_corpus_write_rows_f64(pqv_corpus *corpus, uint64_t row_offset, const double *rows, uint64_t n_rows);
int pqv_corpus_finish(pqv_corpus *corpus, uint64_t n_rows);
/* Host-side helpers of the page-level Parquet reader (N1: parquet_io.py walks the data pages of the embedding leaf itself where
 * it can -- uncompressed or codec-decompressed v1 pages, PLAIN or dictionary-encoded -- instead of materialising Arrow lists):
 *   pqv_parquet_levels_check  decodes an RLE / bit-packed hybrid level run (Parquet "RLE" encoding without the length prefix)
 *                             of n_values levels and checks it WITHOUT storing it: mode 0 -- every level == expect (definition
 *                             levels of a column without nulls); mode 1 -- repetition levels of equal-length lists: level 0 at
 *                             every multiple of `expect` (the list length), 1 elsewhere, the page starting a row.
 *                             0 = as expected, 1 = something else (the caller falls back to the Arrow reader and its messages),
 *                             PQV_ERR_INVALID = malformed run.
 *   pqv_parquet_dict_decode   hybrid-encoded dictionary indices (bit width in the first byte, as in a RLE_DICTIONARY data page)
 *                             -> out[i] = dict[index_i], elem_size 4 or 8 bytes per value.
 * No device is touched. */
int pqv_parquet_levels_check(const uint8_t *buf, uint64_t len, uint32_t bit_width, uint64_t n_values, int mode, uint64_t expect,
                             uint64_t *period_out /* mode 1 with expect == 0: the list length is DISCOVERED (the position of the
                                                     second level 0, or n_values if there is none), written here, then checked */);
int pqv_parquet_dict_decode(const uint8_t *buf, uint64_t len, const void *dict, uint64_t dict_n, uint32_t elem_size,
                            uint64_t n_values, void *out);
/* The page headers of one column chunk, walked from its first byte (Thrift compact PageHeader, parquet.thrift): per page 8
 * ints {type, header bytes, compressed_page_size, uncompressed_page_size, num_values, encoding, definition_level_encoding,
 * repetition_level_encoding}, -1 where the header has no such field.  Stops at len, at max_pages, or once stop_values (> 0)
 * values have been seen in data pages.  (The reference reads pages through the parquet crate: src/ivf/parquet.rs:216-230.) */
/* A run of uncompressed PLAIN v1 data pages of the embedding leaf, from the mapped file to the corpus: per page body (at
 * file_base + body_off[i], body_len[i] bytes) the repetition levels must start a row exactly every `dim` values and every
 * definition level must be max_def (src/ivf/parquet.rs:231-280's checks, on the levels); the n_values[i] values behind the level
 * runs go to rows first_value[i] / dim .. through the pinned staging buffers like pqv_corpus_write_rows (f64 != 0: Float64
 * values, narrowed on the device).  Returns 0, a negative error, or 1 with *bad_page set when page i is not such a page. */
int pqv_corpus_write_plain_pages(pqv_corpus *corpus, const uint8_t *file_base, const uint64_t *body_off, const uint32_t *body_len,
                                 const uint64_t *first_value, const uint32_t *n_values, uint32_t n_pages, uint32_t dim,
                                 uint32_t max_def, int f64, uint32_t *bad_page);
int pqv_parquet_page_headers(const uint8_t *buf, uint64_t len, uint64_t stop_values, uint32_t max_pages, int32_t *out, uint32_t *n_pages);
/* Adopt an existing device buffer [n, dim] f32 on `device` (borrowed; caller keeps it
 * alive and frees it). */
int pqv_corpus_from_device(int device, const void *d_rows, uint64_t n, uint32_t dim,
                           pqv_corpus **out);
uint64_t pqv_corpus_rows(const pqv_corpus *corpus);
uint32_t pqv_corpus_dim(const pqv_corpus *corpus);
int      pqv_corpus_device(const pqv_corpus *corpus);
/* Gather rows (file row ordinals) back to the host: out [m, dim]. */
int pqv_corpus_fetch_rows(const pqv_corpus *corpus, const uint32_t *rows, uint64_t m,
                          float *out);
void pqv_corpus_free(pqv_corpus *corpus);

/* ---- index build ---------------------------------------------------------------------
 * Replaces build_ivf_index(&Embeddings, IvfBuildConfig{n_clusters, max_iters, seed})
 * (src/ivf/index.rs:152-214) including k_means (:323-457), sample_embeddings (:222-242)
 * and the final assignment (:189-206).
 *   n_clusters == 0  => ceil(sqrt(n))                     (:161-167)
 *   workers          => the `available_parallelism()` the reference would see; it fixes the
 *                       f32 partial-sum chunking of k-means++ (:259-265,:356-370).
 *                       0 => this host's online CPU count. */
int pqv_index_build(const pqv_corpus *corpus, uint32_t n_clusters, uint32_t max_iters,
                    uint64_t seed, uint32_t workers, pqv_index **out);
/* ---- index append: rows that arrived after the build -----------------------------------
 * The build's last stage (the final assignment of every row to its nearest centroid and the stable per-cluster sort,
 * src/ivf/index.rs:189-206 + :244-257) depends on the centroids and the rows alone, so it can run for new rows under the centroids an
 * index already has: no k-means, the partition stays.  Grow the column with pqv_corpus_create(capacity) + pqv_corpus_append, then
 * append the new range.  Appending onto an index with empty lists (pqv_index_from_parts) indexes a column under a given codebook.
 * Both calls work on the corpus' stream, like pqv_index_build, and return PQV_ERR_INVALID before any device work for a NULL
 * argument, a dimension mismatch, a range that ends past pqv_corpus_rows(corpus) or past 2^32, or a released row-order copy.
 * A searcher is bound to the rows its index covers: pqv_searcher_create still requires a BUILT index to cover exactly the corpus'
 * rows, so after the corpus grew the old index makes no new searcher (searchers made before keep working on the rows they have);
 * make the new searcher from the appended index.  What an old searcher already holds -- its masks, row keys and results -- stays
 * bit for bit what it was however often the corpus grows and whatever is removed or compacted on descendants of its index.  A
 * row mask or row keys MADE on it after the growth are sized by the corpus' CURRENT row count (pqv_corpus_rows now, not at the
 * searcher's creation; the old length is refused); the rows past the searcher's lists are in no list, so their entries are
 * carried and never read.  A first PQV_COSINE call after the growth normalises the rows the searcher has. */

/* nearest_centroid (src/ivf/index.rs:244-257) of corpus rows [first_row, first_row + n_rows) under the index' centroids:
 * cluster_out[i] = argmin_j squared_l2_distance(row, centroid j), strict '<' from +inf in ascending j (lowest index wins a tie,
 * a row no centroid is < +inf from goes to 0).  Host output [n_rows]. */
int pqv_index_assign(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows, uint32_t *cluster_out);
/* A NEW index: the centroids of `index` bit for bit, list c = list c of `index` followed by the rows of
 * [first_row, first_row + n_rows) assigned to c, ascending -- what index.rs:189-206 leaves for these centroids.  `index` is
 * not modified and stays valid (it may be shared with live searchers).  first_row must be at least the index' row bound (largest
 * indexed row id + 1), which keeps every list ascending; rows between the bound and first_row are simply not indexed.
 * n_rows == 0 yields a copy. */
int pqv_index_append(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows, pqv_index **out);
/* ---- index remove and compact: deleted rows leave the lists, then HBM ---------------------
 * pqv_index_remove* is the logical delete.  A NEW index: the centroids of `index` bit for bit, n_clusters unchanged, list c =
 * list c of `index` without the removed rows, order kept (a list that loses every row stays, empty).  Row ids stay what they
 * were and the row bound (largest indexed row id + 1, as append defines it) is carried over, not lowered: ids are never reused
 * and a later pqv_index_append continues where it would have.  `index` is not modified and stays valid (it may be shared with
 * live searchers; their masks and keys remain what they were).  Where nothing is removed the result is a copy.  An unmasked
 * search of the result returns what a search of `index` under the equivalent pqv_row_mask returns -- through every fast path.
 * The three forms differ in how the rows are named:
 *   pqv_index_remove          host bytes, one per row id in [0, n_flags): non-zero removes the row; ids >= n_flags stay.  n_flags
 *                             may be 0 and may exceed every indexed id.  Runs on `device` where it is usable, else on the host
 *                             with the identical result (also under PQV_DEVICE_LISTS=0).
 *   pqv_index_remove_device   the same bytes in device memory of `device` (required); runs on hip_stream and synchronises it.
 *   pqv_index_remove_rows     the row ids themselves: any order, duplicates allowed, ids that are not indexed ignored.
 * PQV_ERR_INVALID before any device work: a NULL index or out, NULL flags / rows with a non-zero count, n_flags above 2^32.
 *
 * pqv_index_compact is the vacuum.  With M = the rows in the lists of `index` (each below pqv_corpus_rows(corpus) and indexed
 * at most once, else PQV_ERR_INVALID), the new id of row r is its rank in M.  *corpus_out is made like
 * pqv_corpus_create(device of corpus, max(capacity_rows, |M|), dim) and holds the |M| rows of M in ascending old id, bit for
 * bit; *index_out has the centroids bit for bit and every list with the rank applied element by element (monotone: positions
 * and order are preserved), row bound |M|, and is a permutation of the new corpus' rows by construction.  old_row[j] (host,
 * [|M|] -- pqv_index_n_rows(index) entries suffice --, may be NULL) is the old id of new row j: attached columns are re-made as
 * column[old_row].  Works on the corpus' stream; validation as for append (NULLs, dimension mismatch, a released row-order
 * copy).  Neither input is modified. */
int pqv_index_remove(const pqv_index *index, int device, const uint8_t *remove, uint64_t n_flags, pqv_index **out);
int pqv_index_remove_device(const pqv_index *index, int device, const void *d_remove, uint64_t n_flags, void *hip_stream, pqv_index **out);
int pqv_index_remove_rows(const pqv_index *index, int device, const uint32_t *rows, uint64_t m, pqv_index **out);
int pqv_index_compact(const pqv_index *index, const pqv_corpus *corpus, uint64_t capacity_rows,
                      pqv_corpus **corpus_out, pqv_index **index_out, uint32_t *old_row /* host [kept rows], may be NULL */);
/* Phase wall times of the calling thread's last pqv_index_build / pqv_index_build_host / pqv_kmeans (bench records):
 * out[0] k-means++ seconds, [1] Lloyd seconds, [2] Lloyd iterations run, [3] final assignment seconds (device work +
 * download), [4] host inverted-list build seconds, [5] 1 if the final assignment ran through the MFMA screen, [6] same for
 * the Lloyd assignments, [7] sample rows, [8] summed HIP-event seconds of the assign_wide_kernel launches of the final
 * assignment (0 where another form ran), [9] their count; entries beyond n are not written. */
int pqv_index_build_stats(double *out, uint32_t n);
/* ONE k-means++ pick (src/ivf/index.rs:354-390) over given minima, taken the way the build's device rounds take it (kernels_kpp.hip):
 * *total = the `workers` chunks' sequential f32 sums joined in ascending order (:356-370), *pick = the first slot whose sequential f32
 * cumulative sum reaches draw * total (:373-383).  A test entry point: *status 0 = decided; otherwise the reason the build hands the
 * round to its host walk (1 total not positive or not finite, 2 a value that is not a finite non-negative number, 3 no slot reaches the
 * threshold) and *pick is not written.  n in [1, 57344]; workers 0 => this host's online CPU count. */
int pqv_kpp_pick(int device, const float *minima, uint32_t n, uint32_t workers, float draw, uint64_t *pick, float *total,
                 uint32_t *status);
/* Host-pointer form with the reference's exact argument shape: uploads, builds, frees. */
int pqv_index_build_host(int device, const float *data, uint64_t data_len, uint32_t dim,
                         uint32_t n_clusters, uint32_t max_iters, uint64_t seed,
                         uint32_t workers, pqv_index **out);
/* k_means alone (src/ivf/index.rs:323-457) over a resident matrix; centroids [k*dim] and
 * assignments [n] are host outputs; iters_run may be NULL. */
int pqv_kmeans(const pqv_corpus *sample, uint32_t k, uint32_t max_iters, uint64_t seed,
               uint32_t workers, float *centroids, uint32_t *assignments,
               uint32_t *iters_run);

/* ---- index blob ----------------------------------------------------------------------
 * IvfIndex::to_bytes / from_bytes (src/ivf/index.rs:65-128); byte-identical layout. */
int  pqv_index_from_bytes(const uint8_t *bytes, size_t len, pqv_index **out);
int  pqv_index_to_bytes(const pqv_index *index, uint8_t **buf, size_t *len);
void pqv_bytes_free(uint8_t *buf);
/* Assemble from parts (what IvfIndex{..} literal construction does in index.rs:497-502). */
int  pqv_index_from_parts(uint32_t dim, uint32_t n_clusters, const float *centroids,
                          const uint64_t *list_off /*[n_clusters+1]*/,
                          const uint32_t *list_rows, pqv_index **out);
uint32_t pqv_index_dim(const pqv_index *index);              /* IvfIndex::dim() :53 */
uint32_t pqv_index_n_clusters(const pqv_index *index);
uint64_t pqv_index_n_rows(const pqv_index *index);           /* sum of list lengths   */
/* The row bound: largest indexed row id + 1 as a build, an append, a remove (which carries it over, never lowers it) or a compact
 * left it; for an index from bytes or parts the largest id its lists hold + 1 (one host scan on first use); 0 for empty lists or
 * where the lists could not be read (pqv_last_error).  What pqv_index_append starts at and what a table spaces its files by. */
uint64_t pqv_index_row_bound(const pqv_index *index);
const float    *pqv_index_centroids(const pqv_index *index); /* [n_clusters*dim]      */
const uint64_t *pqv_index_list_offsets(const pqv_index *index); /* [n_clusters+1]     */
const uint32_t *pqv_index_list_rows(const pqv_index *index); /* lists, concatenated   */
void pqv_index_free(pqv_index *index);

/* ---- searching -----------------------------------------------------------------------
 * Binds an index to the resident column on the corpus' GPU: uploads centroids + lists and
 * (by default) lays the rows out cluster-contiguously so that a probed inverted list is
 * one sequential HBM range. */
int  pqv_searcher_create(const pqv_index *index, pqv_corpus *corpus, uint32_t flags,
                         pqv_searcher **out);
void pqv_searcher_free(pqv_searcher *searcher);
/* A table of indexed files on one GPU (src/df_vector/index_exec.rs:85-164 on one device): file f's rows are corpus rows
 * [row_base[f], row_base[f] + bound_f), bound_f = pqv_index_row_bound(indexes[f]) (largest indexed row id + 1, carried over by
 * pqv_index_remove: pqv_index_n_rows for a built or appended index, more after a remove, whose surviving rows keep their ids --
 * a file that had a DELETE stays in its table, the removed rows' slots are never candidates); its index' row ids are local to
 * the file and below bound_f.  Returns an ordinary
 * pqv_searcher on which nprobe means "per file": a query probes the first min(nprobe, kc_f) centroids of each file's
 * find_closest_centroids, reported as global list ids cluster_base[f] + c, file after file (P = the sum of those counts).  The
 * candidate sequence is file 0's candidate_rows, then file 1's, ... with rows shifted by row_base; top-k orders by (distance,
 * position in that sequence), as per-file searches merged with pqv_merge_topk.  Row ranges must increase without overlapping
 * (row_base[f + 1] >= row_base[f] + bound_f) and lie inside the corpus; all dims are equal.  P > 1024: as min(nprobe, n_clusters) > 1024 today.
 * max_candidates > 0 returns PQV_ERR_UNSUPPORTED on a table created without PQV_TABLE_CAP_ROUND_ROBIN.  With that flag the cap is
 * the reference's (exec.rs:207-245): file f of a query considers the first t_f of its c_f candidates, t_f being what
 * CandidateCursor::next_batch(max_candidates) of a fresh cursor over the files (access.rs:214-242, file 0 first) takes from it --
 * pqv_round_robin_quota.  Positions in the file-major sequence and the (distance, position) order stay as they are; only the
 * considered set shrinks.  n_candidates stays the count before the cap; embeddings_fetched advances by min(max_candidates, total).
 * On a one-file table the cap is a prefix, as on an ordinary searcher. */
int pqv_table_searcher_create(const pqv_index *const *indexes, uint32_t n_files, const uint64_t *row_base,
                              pqv_corpus *corpus, uint32_t flags, pqv_searcher **out);
/* 1 for ordinary searchers; row_base / cluster_base (each [n_files], may be NULL) for tables. */
int pqv_searcher_files(const pqv_searcher *searcher, uint32_t *n_files, uint64_t *row_base, uint32_t *cluster_base);
/* Host only: quota[f] = the candidates CandidateCursor::next_batch(max_candidates) of a fresh cursor takes from file f, whose
 * candidate count is counts[f] (access.rs:214-242); max_candidates == 0: no cap (quota = counts).  The per-file quotas of a
 * PQV_TABLE_CAP_ROUND_ROBIN table, for hosts that build their own access plans. */
int pqv_round_robin_quota(const uint64_t *counts, uint32_t n_files, uint64_t max_candidates, uint64_t *quota);

/* Tunables of one searcher (all optional; the defaults are the measured dispatch rules of DESIGN.md 5 / DESIGN_HISTORY.md 5.1c-f).
 * The reference has no such knobs -- its topk() is one fixed loop (src/ivf/search.rs:112-127) -- so nothing here
 * changes results, only which kernels produce them; tests use it to force every path through the same oracle.
 *   "rerank_mode"   0 by rule, 1 streaming kernel, 2 batched tile path
 *   "tile_filter"   MFMA lower-bound screen in the batched path: 0 off, 1 by rule, 2 forced
 *   "filter_variant" 1 = one 16-query group per block instead of the wide kernel
 *   "cand_cap"      candidate-buffer entries per query of the wide screened path (0 = by rule: 2048, 8192 for k > 32)
 *   "screen_f16"    f16 screen operands where the data allows (default 1)
 *   "seed_rows", "wide_rows", "tile_rows"   rows sampled for thresholds / per block (0 = by rule)
 *   "running_thr"   running thresholds of the wide kernel (default 1)
 *   "defer"         k > 64 on the wide screened path: survivors of the screen are appended with the distance bounds their
 *                   screen score gives and evaluated after the filter, only where the k-th smallest upper bound leaves them
 *                   (default 1; 0 = every survivor is evaluated by the streaming wave)
 *   "quad_xcd"      quad-to-XCD affinity of the wide kernels (-1 by rule)
 *   "wide_waves"    waves per block of the wide kernel: 0 by rule, 4 or 8
 *   "quad_width"    queries per quad of the wide kernel (0 by rule; a multiple of 32)
 *   "screen_i8"     int8 screen operands for rows of a multiple of 256 dims (default 1)
 *   "min_blocks"    workgroups the wide kernel's rows-per-block rule aims for on small batches (0 by rule)
 *   "pair_prune"    int8 path: skip (query, list) pairs whose centre-distance bound already exceeds the query's threshold
 *                   (default 1)
 *   "i8_form"       int8 images: 0 by rule -- the per-list residual (one query image per probed pair) where the lists' own
 *                   scales are >= 1.3x the scale one centre for the whole corpus would get, else the one-centre form (one
 *                   image per query) --, 1 one centre, 2 residual; the int8 copy is rebuilt on the next call
 *   "single_bucket" a single-query call is bucketed by the probe merge itself (two launches less).  1 (default) and 3: the
 *                   probe joins that launch too wherever there are at most 4096 centroids (probe_single_kernel); 2: the
 *                   bucketing only, the probe keeps its own launch; 0: the general three-launch pair sort
 *   "seed_refine"   exact distances of the rows behind the k selected seed bounds replace the k-th bound as the first
 *                   threshold (k <= 16; default 1)
 *   "item_grid"     wide kernel grid: 1 = one workgroup per (quad, existing row chunk) for the 4-wave blocks (default),
 *                   2 = for the 8-wave blocks too, 0 = (chunks of the longest list) x quads
 *   "chunk_major"   order of those work items: 1 (default) = row chunk 0 of every quad, then chunk 1, ... -- a query's
 *                   thresholds have seen a piece of each of its lists before the bulk is screened; 0 = list by list
 *   "probe_rows"    batched centroid probe (a lane per centroid): 1 for batches of >= 8 queries (default), 2 always,
 *                   0 = the per-query stream over the centroid table
 *   "probe_screen"  that batched probe screened on the matrix cores (probe_screen_kernel + probe_resolve_kernel: an f16 contraction
 *                   against centroid images, exact chains only for the centroids its bounds cannot exclude; same results): 1 by
 *                   rule (default: >= 128 queries, >= 256 centroids, nprobe <= n_clusters / 4, no table, not PQV_DOT), 2 for every
 *                   batch the kernels support, 0 off.  The centroid images are made when the searcher is created, or by the
 *                   first non-zero setting of this option where PQV_PROBE_SCREEN=0 kept creation from making them
 *   "wide_quads"    int8 path, batches: lists probed by 97..160 queries in ONE quad of the wide-quad instance (32-row tiles, one
 *                   8-wave block per CU) instead of two regular quads.  1 (default): by the PREVIOUS batch's shape -- regular quads
 *                   only while most rows of the popular lists sit in lists of > 160 pairs (clustered query loads); 2 always; 0 never
 *   "wide_quad_rows" rows per block of that instance (0 by rule: 8192; 2048 for the list form below)
 *   "list_once"     int8 path, batches, dims 256 / 512 / 768, no deferred evaluation: 1 = lists probed by more than 96 queries run in
 *                   list_filter_kernel -- 32 rows per wave stationary in registers, ALL the list's pairs (quads of up to 1024) streamed
 *                   past them: every such list is read once.  0 (default): measured slower than the wide-quad instance
 *   "xcd_items"     a level's work items are filled column by column of an 8-column layout, so that the quads of one list run
 *                   back to back on one XCD and share its rows through that L2: 1 (default) = in the table that has several
 *                   quads per list, 3 = in both tables, 0 = off
 *   "fork_wide"     the wide-quad launch on a side stream of the call's lane: 0 off (default), 1 regular instance first, 2 wide first
 *   "pf96"          f16 96-query form on rows of <= 128 dims: all of the next tile's operands are requested behind the current tile's
 *                   MFMAs (1 = for lists of <= 2048 rows on average (default), 2 always, 0 never)
 *   "static_dim"    int8 path, batches, k <= 64: 1 (default) = rows of 768 dims run the screen instances that have the row length compiled
 *                   in (K loops unrolled, every A-operand read at a lane address + immediate; same results); 0 = the run-time row length
 *                   everywhere (A/B runs)
 *   "drain_min"     queued survivors that start a batch of exact evaluations before a wave's last tile (0 = 64)
 *   "partition_blocks" pqv_topk_partition: blocks per query of partition_stream_kernel (0 = by rule, from nq, k and the partition's
 *                   rows; at most 4096).  pqv_range_search_partition: the same, by rule from the group and its longest sequence
 *   "partition_range_bytes" pqv_range_search_partition: the byte budget of one group's hit segments (0 = 1 GiB)
 * The same names, upper-cased with a PQV_ prefix, are read from the environment ONCE when a searcher is created
 * (profiling scripts). */
int pqv_searcher_set_option(pqv_searcher *searcher, const char *name, int64_t value);
/* Which kernels a pqv_topk_device call of this shape would run on this searcher (one line of text, for bench
 * records): written NUL-terminated into buf (truncated to len).  PQV_COSINE: the query normalisation, then the dispatch of the
 * searcher's cosine layout (of this searcher's L2 dispatch while that layout is not built). */
int pqv_searcher_describe(const pqv_searcher *searcher, uint32_t nq, uint32_t k, uint32_t nprobe, int metric,
                          char *buf, size_t len);
/* Device memory held for this searcher, in bytes: the corpus' row-order copy (0 once released), the IVF-ordered
 * f32 rows, the blocked screen-operand copy, and everything else (centroids, lists, norms, scratch lanes).  Once the PQV_COSINE
 * layout is built its buffers are added to the same four classes (its normalised rows to the first or the second). */
int pqv_searcher_footprint(const pqv_searcher *searcher, uint64_t *row_order_bytes, uint64_t *ivf_rows_bytes,
                           uint64_t *blocked_bytes, uint64_t *other_bytes);

/* IvfIndex::find_closest_centroids (src/ivf/index.rs:130-149): clusters_out has room for
 * min(nprobe, n_clusters); *n_out receives the count. */
int pqv_probe(const pqv_searcher *searcher, const float *query, uint32_t query_len,
              uint32_t nprobe, uint32_t *clusters_out, uint32_t *n_out);
/* IvfIndex::candidate_rows (src/ivf/index.rs:57-63): library buffer, probe-rank major. */
int  pqv_candidate_rows(const pqv_searcher *searcher, const float *query, uint32_t query_len,
                        uint32_t nprobe, uint32_t **rows, uint64_t *n_rows);
void pqv_rows_free(uint32_t *rows);

/* topk() (src/ivf/search.rs:83-142) for nq queries at once: probe, re-rank every
 * candidate, keep the k smallest by (d2, candidate position), order ascending.
 *   queries      host [nq, query_len]; query_len must equal the index dim (:91-98)
 *   max_candidates  0 => none; else the CandidateCursor cap (src/df_vector/access.rs:
 *                   214-242, single file): only the first max_candidates candidates in
 *                   probe-rank order are considered
 *   metric       PQV_L2SQ_REF4 (TopkBuilder), PQV_L2SQ_SEQ (VectorTopKExec) or PQV_COSINE (0.5f * d2 of the normalised
 *                vectors: see PQV_COSINE)
 *   sqrt_out     nonzero => dist = sqrt(d2) as TopkBuilder returns (:133); 0 => d2 (ignored for PQV_COSINE)
 *   row_idx/dist host [nq*k]; entries past n_found[q] are 0xFFFFFFFF / +inf
 * Ties: when two of a query's k results (or the k-th and the runner-up) have EQUAL output
 * distance, which rows survive and in what order is an artefact of Rust's BinaryHeap sift
 * history (search.rs:113-140).  pqv_topk detects that on the device and replays exactly those
 * queries through the same heap mechanics on the host (distances still computed on the GPU),
 * so its results equal the reference's in every non-NaN case.  pqv_topk_device never leaves
 * the GPU: it returns the k smallest by (d2, candidate position), identical to the reference
 * whenever no such tie exists.  (k == 1024, the largest supported, has no runner-up slot: a tie between the
 * 1024th result and the first excluded candidate is then not detected.)
 *   n_found      host [nq] (may be NULL)
 *   n_candidates host [nq] (may be NULL): sum of the probed lists' lengths, before the cap */
int pqv_topk(const pqv_searcher *searcher, const float *queries, uint32_t nq,
             uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates,
             int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found,
             uint64_t *n_candidates);

/* Device-resident form: queries and outputs are device pointers on the searcher's GPU,
 * work is enqueued on `hip_stream` (a hipStream_t passed as void*; NULL = the searcher's
 * own NON-BLOCKING stream -- NOT HIP's legacy default stream, whose handle is also 0: a caller
 * whose next operation runs on the default stream (torch.cuda.current_stream() outside a stream
 * context) must pass an explicit stream -- hipStreamLegacy, ((hipStream_t)1), names the default stream itself -- or
 * synchronise) and the call returns without
 * synchronising.  d_n_found / d_n_candidates may be NULL.  This is what bench.py times.  PQV_COSINE (see there): n(q) is computed
 * on `hip_stream` into the searcher's scratch, the halving happens in the final merge; the first cosine call on a searcher builds
 * its cosine layout and synchronises once. */
int pqv_topk_device(const pqv_searcher *searcher, const void *d_queries, uint32_t nq,
                    uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric,
                    int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found,
                    void *d_n_candidates, void *hip_stream);

/* The same, plus d_tie_flags (device u32 [nq]): 1 for every query two of whose k results (or the k-th and the
 * runner-up) have EQUAL output distance -- exactly the queries for which the reference's survivors / order depend on
 * BinaryHeap history (src/ivf/search.rs:113-140) and pqv_topk_device's (d2, position) order may differ from it.
 * Everything stays asynchronous; a caller that needs the reference's answer under ties re-submits the flagged
 * queries to pqv_topk, which replays the heap exactly.  (The kernels then work with k + 1 entries: k <= 1023.) */
int pqv_topk_device_flags(const pqv_searcher *searcher, const void *d_queries, uint32_t nq, uint32_t k,
                          uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out, void *d_row_idx,
                          void *d_dist, void *d_n_found, void *d_n_candidates, void *d_tie_flags, void *hip_stream);

/* Range search: EVERY candidate within `radius` of each query, for nq queries in one call.
 *   candidates   candidate_rows(q, nprobe) (probe-rank order, list order inside a list), the first max_candidates of them
 *                when max_candidates > 0 (as pqv_topk); a candidate's position is its index in that sequence.  nprobe is
 *                clamped to n_clusters and may exceed 1024.
 *   distance     d2 of `metric` (bit-identical to pqv_topk's); out = sqrt_out ? sqrt(d2) (correctly rounded) : d2.  PQV_COSINE:
 *                d2 of the normalised vectors, out = 0.5f * d2 whatever sqrt_out (see PQV_COSINE).
 *   hit          out <= radius (inclusive, on the output scale).  A NaN distance is never a hit; radius = +inf keeps every
 *                other candidate, a negative radius none; a NaN radius is PQV_ERR_INVALID ("radius must not be NaN").
 *   order        ascending by (d2, position): unique per query, independent of scheduling.
 *   max_results  > 0: only the first max_results hits in that order are returned.  Where the cut falls inside a group of
 *                equal distances the kept rows follow (d2, position) -- pqv_topk, which follows the reference's heap
 *                history on ties, may keep others.
 * Output (CSR): query q's hits are row_idx / dist [lims[q], lims[q+1]); *lims [nq + 1] (lims[0] = 0, allocated also for
 * nq = 0), *row_idx and *dist [lims[nq]] are library buffers released with pqv_range_free.  n_within host [nq] (may be
 * NULL): the full hit count (before max_results); n_candidates host [nq] (may be NULL): sum of the probed lists' lengths,
 * before the cap.  Counters advance as for a pqv_topk call of the same shape; the searcher's other state is untouched. */
int  pqv_range_search(const pqv_searcher *searcher, const float *queries, uint32_t nq, uint32_t query_len,
                      float radius, uint32_t nprobe, uint64_t max_candidates, uint64_t max_results,
                      int metric, int sqrt_out, uint64_t **lims, uint32_t **row_idx, float **dist,
                      uint64_t *n_within, uint64_t *n_candidates);
void pqv_range_free(uint64_t *lims, uint32_t *row_idx, float *dist);

/* Row-masked search: top-k and range search restricted to a set of rows -- the `WHERE <predicate>` of
 * `SELECT .. WHERE <predicate> ORDER BY array_distance(col, q) LIMIT k`, which the reference evaluates inside the scan, after
 * candidate pruning and before the heap (src/df_vector/exec.rs:207-277) -- and equally deleted rows or a tenant's rows.
 *
 * A row mask is one bit per row of the searcher's corpus: bit r belongs to the row a call reports as row_idx == r (a file row
 * of a plain searcher, a corpus row of a table searcher).  It is made for ONE searcher, from `allowed` [n_rows] bytes (nonzero =
 * allowed; n_rows must equal pqv_corpus_rows of the searcher's corpus, else PQV_ERR_INVALID "row mask has N rows, the corpus has
 * M"), and is immutable.  Rows that belong to no inverted list are ignored; pqv_row_mask_count is the number of allowed rows
 * that belong to one.  pqv_row_mask_from_device reads device bytes (u8 [n_rows], e.g. a torch.bool tensor) on hip_stream (NULL:
 * the searcher's) and is complete on return.  Any thread may use a mask; mask and searcher may be freed in either order; the
 * caller keeps a mask alive until the work enqueued with it has completed, as with its query buffers.
 *
 * A masked call behaves as the unmasked call of the same arguments, except:
 *   candidates   the unmasked call's sequence (candidate_rows order; file-major on a table), cut by max_candidates / the table's
 *                round-robin quotas exactly as there, BEFORE the mask is looked at; the considered rows are the allowed rows
 *                among the capped candidates, at their UNMASKED positions.  Top-k and range order by (d2, position); tie rules
 *                (the host form replays the reference's heap over the considered rows in arrival order; the device form flags),
 *                sqrt_out, max_results and the PQV_COSINE halving are unchanged.
 *   counts       n_candidates and the candidate_rows counter stay the counts before cap and mask; embeddings_fetched advances
 *                by the considered rows (the reference's counter after the filter); n_found may be below k, or 0 (rows
 *                0xFFFFFFFF, distance +inf); n_within counts masked hits.
 *   equivalence  with max_candidates == 0 on a plain searcher the call returns, bit for bit, what the unmasked call returns on a
 *                searcher over pqv_index_from_parts(dim, centroids, [list intersected with the allowed rows, for each list])
 *                and the same corpus -- rows, distances, n_found, tie flags -- n_candidates excepted.
 *   path         always the exact streaming pass (masked_stream_kernel): no searcher option changes a masked result, and rows the
 *                mask excludes are never read.  k > 1024 or more than 1024 probed lists: pqv_topk_masked goes through the host heap
 *                like pqv_topk; the device form reports PQV_ERR_UNSUPPORTED like pqv_topk_device.
 * Errors (PQV_ERR_INVALID): "row mask must not be NULL", "row mask belongs to another searcher".
 * pqv_topk_masked_device: d_tie_flags may be NULL (then k <= 1024, else k <= 1023). */
typedef struct pqv_row_mask pqv_row_mask;
int      pqv_row_mask_create(const pqv_searcher *searcher, const uint8_t *allowed, uint64_t n_rows, pqv_row_mask **out);
int      pqv_row_mask_from_device(const pqv_searcher *searcher, const void *d_allowed, uint64_t n_rows, void *hip_stream,
                                  pqv_row_mask **out);
uint64_t pqv_row_mask_rows(const pqv_row_mask *mask);
uint64_t pqv_row_mask_count(const pqv_row_mask *mask);
void     pqv_row_mask_free(pqv_row_mask *mask);
int pqv_topk_masked(const pqv_searcher *searcher, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                    uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                    uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_masked_device(const pqv_searcher *searcher, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                           uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out, void *d_row_idx,
                           void *d_dist, void *d_n_found, void *d_n_candidates, void *d_tie_flags, void *hip_stream);
int pqv_range_search_masked(const pqv_searcher *searcher, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                            uint32_t query_len, float radius, uint32_t nprobe, uint64_t max_candidates, uint64_t max_results,
                            int metric, int sqrt_out, uint64_t **lims, uint32_t **row_idx, float **dist,
                            uint64_t *n_within, uint64_t *n_candidates);

/* Predicate masks: the WHERE clause evaluated on the GPU.  A pqv_column is one scalar column resident on one GPU beside the
 * embedding column: one value per corpus row (PQV_COL_*), optionally validity bytes (u8 [n_rows], 0 = NULL).
 * pqv_column_upload copies host arrays; pqv_column_from_device borrows device arrays, as pqv_corpus_from_device does (the caller
 * keeps them alive and unchanged).  pqv_row_mask_from_predicates evaluates a predicate over such columns into an ordinary
 * immutable pqv_row_mask, good for every masked entry point (plain and table searchers, every layout, every metric).  Nothing
 * of size O(n_rows) crosses PCIe: the leaf table and the program go in, the 8-byte allowed total comes out.
 *
 * A predicate is n_leaves <= 32 leaves and a postfix program over them (program_len <= 63 bytes: 0..31 pushes leaf i,
 * PQV_PRED_AND / PQV_PRED_OR replace the two top values; stack depth <= 32; exactly one value is left).  Leaf i is
 * (columns[i], ops[i], operands[2 i], operands[2 i + 1]):
 *   truth      true on a row iff  valid && (cmp(x) != negate),  negate = ops[i] & PQV_OP_NOT.  PQV_OP_IS_NULL is
 *              (!valid) != negate; a column without validity bytes is never NULL.  PQV_OP_MASK is  bit != negate  of masks[i],
 *              an existing row mask of THIS searcher (columns[i] is ignored and may be NULL).
 *   operands   slot 0 (and slot 1 for PQV_OP_BETWEEN: lo <= x && x <= hi) holds the bits of an int64_t for I32 / I64 columns
 *              and of a double for F32 / F64 columns.  Integer columns compare in i64 (never through floating point: 2^53
 *              and 2^53 + 1 stay distinct); float columns compare in f64 (an f32 value is widened, which is exact) with IEEE
 *              rules: NaN makes every op false except NE -- so a negated LT is true on NaN -- and -0.0 == 0.0.
 *   combining  AND / OR are two-valued and there is no NOT operator: negation exists on leaves only (push NOT down with De
 *              Morgan).  With `valid` gating every leaf this equals SQL's three-valued logic followed by "NULL counts as
 *              false"; a negated membership test (an AND of negated EQ leaves) drops NULL rows, as SQL's NOT IN does.
 *   columns    have pqv_corpus_rows rows and live on the searcher's device; row r is the row a call reports (a corpus row of a
 *              table searcher).  Rows outside every file or list are evaluated -- pqv_row_mask_to_bytes shows them -- and
 *              ignored by searches and pqv_row_mask_count, as for every mask.
 *   completion work is enqueued on hip_stream (NULL: the searcher's) and complete on return; columns and MASK leaves are only
 *              read during the call.
 * pqv_predicate_check validates a program on the host (no device) and reports its deepest stack in *max_depth (may be NULL).
 * pqv_row_mask_to_bytes writes allowed[r] = 1 where row r is allowed, else 0, for every corpus row, from any mask: it downloads
 * the mask's row-order device bitset (n_rows / 8 bytes) and expands it, for a byte-made mask too.
 * Errors (PQV_ERR_INVALID, before any device use where the arguments allow it): "predicate program is empty", "predicate
 * program is malformed" (unknown byte, leaf index >= n_leaves, underflow, overflow, more than one value left), "predicate has N
 * leaves, at most 32", "unknown column type", "unknown predicate op", "column has N rows, the corpus has M", "column is on device
 * D, the searcher on device E", "predicate leaf I has no column", "row mask belongs to another searcher" (MASK leaves). */
#define PQV_COL_I32 0
#define PQV_COL_I64 1
#define PQV_COL_F32 2
#define PQV_COL_F64 3
typedef struct pqv_column pqv_column;
int      pqv_column_upload(int device, int dtype, const void *values, const uint8_t *valid, uint64_t n_rows, pqv_column **out);
int      pqv_column_from_device(int device, int dtype, const void *d_values, const void *d_valid, uint64_t n_rows,
                                pqv_column **out);
uint64_t pqv_column_rows(const pqv_column *column);
int      pqv_column_dtype(const pqv_column *column);
int      pqv_column_device(const pqv_column *column);
void     pqv_column_free(pqv_column *column);
#define PQV_OP_EQ 0
#define PQV_OP_NE 1
#define PQV_OP_LT 2
#define PQV_OP_LE 3
#define PQV_OP_GT 4
#define PQV_OP_GE 5
#define PQV_OP_BETWEEN 6
#define PQV_OP_IS_NULL 7
#define PQV_OP_MASK 8
#define PQV_OP_NOT 0x100
#define PQV_PRED_AND 0x80
#define PQV_PRED_OR  0x81
int pqv_predicate_check(const uint8_t *program, uint32_t program_len, uint32_t n_leaves, uint32_t *max_depth);
int pqv_row_mask_from_predicates(const pqv_searcher *searcher, uint32_t n_leaves, const pqv_column *const *columns,
                                 const pqv_row_mask *const *masks, const uint32_t *ops, const uint64_t *operands,
                                 const uint8_t *program, uint32_t program_len, void *hip_stream, pqv_row_mask **out);
int pqv_row_mask_to_bytes(const pqv_row_mask *mask, uint8_t *allowed, uint64_t n_rows);

/* Per-query key filters: one batched search in which every query has its own `key_column = ?` -- a tenant, a user, a
 * collection -- where a row mask is ONE filter for the whole batch.
 *
 * A pqv_row_keys is a resident INTEGER column (PQV_COL_I32 or PQV_COL_I64, one value per corpus row, optional validity bytes)
 * laid out for ONE searcher, plain or table: key_pos[p] = column[row that list position p reports] at the column's own width,
 * beside a validity bitset in a mask's format where the column has validity bytes.  pqv_row_keys_create copies what it needs
 * (the column may be freed or changed afterwards), runs on hip_stream (NULL: the searcher's) and is complete on return; the
 * result is immutable, serves every layout, every metric and every keyed entry point, may be used by any thread, and may be
 * freed before or after its searcher.  Nothing of size O(n_rows) crosses PCIe, except once for the first call that replays a
 * query on the host (tied distances, k > 1024, more than 1024 probed lists).
 *
 * A keyed call is its masked twin with `keys`, `qkeys` (int64_t [nq], one key per query; the device form reads a device array
 * on hip_stream, inside the enqueued work) and `mask` (an optional shared row mask, NULL: none) inserted behind `searcher`.  With
 *     M_q[r] = valid[r] && (int64_t) column[r] == qkeys[q] && (mask ? mask[r] : 1)
 * query q of a keyed call returns, bit for bit, what the masked twin returns for that one query under the mask M_q:
 *   candidates   the unmasked sequence, cut by max_candidates / a table's round-robin quotas BEFORE the filter; the considered
 *                rows are the rows of M_q among the capped candidates, at their UNMASKED positions; order, tie rules (host heap
 *                replay, device tie flags), sqrt_out, max_results and the PQV_COSINE halving are the masked call's.
 *   counts       n_candidates and candidate_rows stay the counts before cap and filter; embeddings_fetched advances by the
 *                considered rows, summed over the batch; n_found may be below k, or 0 (rows 0xFFFFFFFF, distance +inf); n_within
 *                counts the hits in M_q.
 *   comparison   in i64: an I32 column's values are widened, so a query key outside the i32 range matches nothing on an I32
 *                column (it is never truncated).  A NULL row never matches.  Two queries may carry the same key; a key no row
 *                has gives n_found == 0 or an empty range.
 *   path         always the exact streaming pass, as for masks: no searcher option changes a keyed result, and rows the filter
 *                excludes are never read.  k > 1024 or more than 1024 probed lists: pqv_topk_keyed goes through the host heap like
 *                pqv_topk_masked; the device form reports PQV_ERR_UNSUPPORTED like pqv_topk_masked_device.
 * Errors (PQV_ERR_INVALID; NULL handles are checked before any device use): "searcher must not be NULL", "out must not be NULL",
 * "column must not be NULL", "key column must be PQV_COL_I32 or PQV_COL_I64", "column has N rows, the corpus has M", "column is
 * on device D, the searcher on device E", "row keys must not be NULL", "query keys must not be NULL", "row keys belong to
 * another searcher", and the masked calls' own ("row mask belongs to another searcher"). */
typedef struct pqv_row_keys pqv_row_keys;
int      pqv_row_keys_create(const pqv_searcher *searcher, const pqv_column *column, void *hip_stream, pqv_row_keys **out);
uint64_t pqv_row_keys_rows(const pqv_row_keys *keys);
int      pqv_row_keys_dtype(const pqv_row_keys *keys);
void     pqv_row_keys_free(pqv_row_keys *keys);
int pqv_topk_keyed(const pqv_searcher *searcher, const pqv_row_keys *keys, const int64_t *qkeys, const pqv_row_mask *mask,
                   const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates,
                   int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_keyed_device(const pqv_searcher *searcher, const pqv_row_keys *keys, const void *d_qkeys, const pqv_row_mask *mask,
                          const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric,
                          int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates, void *d_tie_flags,
                          void *hip_stream);
int pqv_range_search_keyed(const pqv_searcher *searcher, const pqv_row_keys *keys, const int64_t *qkeys,
                           const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len, float radius,
                           uint32_t nprobe, uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out,
                           uint64_t **lims, uint32_t **row_idx, float **dist, uint64_t *n_within, uint64_t *n_candidates);

/* Per-query filters beyond equality: `key IN (...)` (the groups a user belongs to) and `key BETWEEN ? AND ?` (a window of
 * timestamps, prices, versions) per query of one batch.  A filtered call is its keyed twin with a filter descriptor where the
 * twin has `qkeys`: with F_q(v) the descriptor's test for query q on an i64 value and
 *     M_q[r] = valid[r] && F_q((int64_t) column[r]) && (mask ? mask[r] : 1)
 * query q returns, bit for bit, what the masked twin returns for that one query under the mask M_q -- candidates, counts, path,
 * ties, sqrt_out, max_results, the PQV_COSINE halving, the limits beyond the kernels' lists and the PQV_DOT refusal are the keyed
 * contract above, word for word.
 *   PQV_KEY_EQ     a: int64_t [nq].  key == a[q]: pqv_topk_keyed* exactly.  b is not read.
 *   PQV_KEY_RANGE  a, b: int64_t [nq].  a[q] <= key && key <= b[q], both ends inclusive; a[q] > b[q] matches nothing and is no
 *                  error; [INT64_MIN, INT64_MAX] matches every valid row.
 *   PQV_KEY_IN     a: uint64_t lims [nq + 1], b: int64_t values.  key is one of b[a[q] .. a[q + 1]).  lims[0] == 0, lims does not
 *                  decrease, every query's slice is strictly ascending (sorted, no duplicates) and holds at most PQV_KEY_SET_MAX
 *                  values; an empty slice matches nothing.
 * Comparisons are in i64: an I32 column is widened, never truncated, so a range or a set beyond the i32 values matches nothing
 * there.  A NULL row never matches.  `reserved` must be 0.
 * The host forms validate the descriptor before any device use, ahead of the keyed calls' own checks and in this order
 * (PQV_ERR_INVALID): "filter must not be NULL", "unknown key filter kind N", "query keys must not be NULL" (a, and b where the
 * kind reads it), "query key sets must start at 0 and not decrease", "a query key set takes at most 1024 values", "query key
 * sets must be strictly ascending".  The device form takes a and b as DEVICE arrays read on hip_stream inside the enqueued work,
 * so the call stays asynchronous and a set cannot be validated: the kernels read at most PQV_KEY_SET_MAX values of a slice and
 * never anything outside b[a[q] .. a[q + 1]); for a slice that is longer or not strictly ascending that query's result is
 * unspecified, and every access stays inside the slice. */
#define PQV_KEY_EQ     0
#define PQV_KEY_RANGE  1
#define PQV_KEY_IN     2
#define PQV_KEY_SET_MAX 1024
typedef struct pqv_key_filter {
    uint32_t    kind;      /* PQV_KEY_* */
    uint32_t    reserved;  /* 0 */
    const void *a;
    const void *b;
} pqv_key_filter;
int pqv_topk_filtered(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                      const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates,
                      int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_filtered_device(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_key_filter *filter,
                             const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                             uint64_t max_candidates, int metric, int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found,
                             void *d_n_candidates, void *d_tie_flags, void *hip_stream);
int pqv_range_search_filtered(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_key_filter *filter,
                              const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len, float radius,
                              uint32_t nprobe, uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out,
                              uint64_t **lims, uint32_t **row_idx, float **dist, uint64_t *n_within, uint64_t *n_candidates);

/* Expanding filtered top-k: keep probing until k rows pass the filter.  A selective mask or key filter often leaves fewer than k
 * passing rows in a query's `nprobe` nearest lists; raising nprobe for the whole batch makes every query pay for the worst one.
 * An expanding call lets each query probe further on its own, up to `max_nprobe` lists, decided on the device in one submission.
 *
 * Which filter the call takes:
 *   keys == NULL   filter must be NULL and mask non-NULL: the twin is pqv_topk_masked / pqv_topk_masked_device.
 *   keys != NULL   filter must be non-NULL (PQV_KEY_EQ is the keyed call); mask is the optional shared mask: the twin is
 *                  pqv_topk_filtered / pqv_topk_filtered_device.
 * With M_q the row set of the twin for query q (the mask, or M_q[r] of the keyed / filtered contract above) and
 *     kc = n_clusters, p0 = min(nprobe, kc), P = min(max_nprobe, kc),
 *     cnt_q(p) = the rows of M_q in the first p lists of q's probe order (a row counts whatever its distance is, NaN included),
 *     nprobe_used[q] = the smallest p in [p0, P] with cnt_q(p) >= k, or P if there is none,
 * query q's row_idx, dist, n_found and tie flag are, bit for bit, what the twin returns for that one query with the same arguments,
 * nprobe = nprobe_used[q] and max_candidates = 0 (the probe order is prefix-consistent: the nearest P centroids by (d2, id) begin
 * with the nearest p).  The host form replays flagged queries through the reference heap over that query's first nprobe_used[q]
 * lists, as its twin does.  n_candidates[q] is the summed length of those lists.  max_nprobe == nprobe is the twin call itself.
 * No searcher option changes a result.
 *   counts     as for those nq twin calls: queries advances by nq, candidate_rows by the sum of n_candidates, embeddings_fetched
 *              by the considered rows in the used lists.  The counting pass reads no embedding and counts nothing.
 *   scope      plain searchers, both layouts, PQV_L2SQ_REF4, PQV_L2SQ_SEQ and PQV_COSINE (through the cosine layout, as the
 *              twins).  nprobe_used / d_nprobe_used, n_found, n_candidates and d_tie_flags may be NULL.  The device form is
 *              asynchronous on hip_stream like its twin, with no host synchronisation; device filter arrays are read inside
 *              the enqueued work.
 *   path       the probe ranks P lists per query; a counting pass over the filter's images (1 bit per row of a mask, 4 or 8
 *              bytes per row of a key column) and a select write nprobe_used; ONE exact streaming pass then walks each query's
 *              lists below its own limit.
 *   out of scope  table searchers, PQV_DOT, max_candidates, range search, and -- for the host form too -- k or P beyond the kernels'
 *              lists.  (Expansion with a group column: pqv_topk_distinct_expand below.)
 * Errors, checked in this order, NULL handles before any device use -- PQV_ERR_INVALID: "searcher must not be NULL",
 * "pqv_topk_expand needs a row mask or row keys", "a key filter needs row keys" (filter without keys), "filter must not be NULL"
 * (keys without filter), the filter-descriptor checks of the filtered host form, "max_nprobe must be >= nprobe", then the twin's
 * own ("row mask belongs to another searcher", "k must be > 0", ...).  PQV_ERR_UNSUPPORTED: "pqv_topk_expand does not take table
 * searchers", "PQV_DOT is not supported by pqv_topk_expand", "pqv_topk_expand takes k <= 1024 (1023 with tie flags) and at most
 * 1024 probed lists per query" (both forms; the host form always carries tie flags and does not fall back to the host heap path). */
int pqv_topk_expand(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                    const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t max_nprobe,
                    int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates,
                    uint32_t *nprobe_used);
int pqv_topk_expand_device(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_key_filter *filter,
                           const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                           uint32_t max_nprobe, int metric, int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found,
                           void *d_n_candidates, void *d_nprobe_used, void *d_tie_flags, void *hip_stream);

/* Per-query probe depths for the PLAIN top-k call: every query of a batch walks its own number of lists -- given by the caller (a
 * frontend that batches requests with different nprobe values), or decided on the device from the centroid distances (a query
 * inside a cluster needs its home list and little else; one between clusters needs more).  The call keeps the plain call's
 * screened kernels; a rank nobody walks makes no work item, no seed sample and no pair image.
 *
 * With kc = n_clusters, p0 = min(nprobe, kc), P = min(max_nprobe, kc), c_0 .. c_{P-1} the query's probe order (the P nearest
 * centroids by (d2, id)) and d2_j their probe distances -- the reference chain PQV_L2SQ_REF4 whatever `metric` is; PQV_COSINE: that
 * chain of the normalised query against the normalised centroids, as the cosine probe -- the raw depth r_q is
 *   PQV_DEPTH_GIVEN   depths[q];
 *   PQV_DEPTH_RATIO   the number of j < P with d2_j <= t, t the single f32 product d2_ratio * d2_0 (no contraction).  d2_ratio is on
 *                     the SQUARED scale.  A NaN on either side compares false: d2_0 == 0 with d2_ratio == +inf gives t = NaN and
 *                     r_q = 0.  The distances ascend, so the counted ranks are a prefix.
 * and nprobe_used[q] = min(max(r_q, p0), P): nprobe is the floor and max_nprobe the ceiling in both kinds; a given depth of 0 or
 * above P is clamped, not refused (the device form cannot read the array).
 * Query q's row_idx, dist, n_found and tie flag are, bit for bit, what pqv_topk / pqv_topk_device / pqv_topk_device_flags returns
 * for that one query at nprobe = nprobe_used[q] and max_candidates = 0 (no new result is defined: the probe order is
 * prefix-consistent and candidate positions are prefix sums in it).  The host form replays flagged queries through the reference
 * heap over the query's first nprobe_used[q] lists.  n_candidates[q] is the summed length of those lists.  No searcher option changes
 * a result.
 *   counts     as for those nq single calls: queries advances by nq, candidate_rows and embeddings_fetched by the sum of
 *              n_candidates.
 *   scope      plain searchers, both layouts; PQV_L2SQ_REF4, PQV_L2SQ_SEQ and PQV_COSINE; k <= 1024 (1023 for the host form and for
 *              the device form with tie flags); P <= 1024.  nprobe_used / d_nprobe_used, n_found, n_candidates and d_tie_flags may be
 *              NULL.  GIVEN: depths is a host array in the host form and a device array, read inside the enqueued work, in the device
 *              form.  The device form is asynchronous on hip_stream, with no host synchronisation.
 *   out of scope  a depth combined with a mask, keys, a distinct or grouped call (those expand by counting: pqv_topk_expand,
 *              pqv_topk_distinct_expand); range search; max_candidates; table searchers; PQV_DOT.
 * Errors, NULL handles before any device use -- PQV_ERR_INVALID: "searcher must not be NULL", "depth must not be NULL",
 * "max_nprobe must be >= nprobe", "unknown depth kind", "depths must not be NULL" (GIVEN), "d2_ratio must be >= 1 and not NaN"
 * (RATIO), then the plain call's own ("k must be > 0", ...).  PQV_ERR_UNSUPPORTED: "pqv_topk_depth does not take table searchers",
 * "PQV_DOT is not supported by pqv_topk_depth", "pqv_topk_depth takes k <= 1024 (1023 with tie flags) and at most 1024 probed lists
 * per query". */
#define PQV_DEPTH_GIVEN 0
#define PQV_DEPTH_RATIO 1
typedef struct pqv_probe_depth {
    uint32_t    kind;        /* PQV_DEPTH_GIVEN | PQV_DEPTH_RATIO */
    uint32_t    max_nprobe;  /* >= nprobe; the lists the probe ranks per query */
    float       d2_ratio;    /* RATIO: >= 1, may be +inf, not NaN; on the SQUARED scale */
    const void *depths;      /* GIVEN: u32 [nq], host (host form) / device (device form) */
} pqv_probe_depth;
int pqv_topk_depth(const pqv_searcher *searcher, const pqv_probe_depth *depth, const float *queries, uint32_t nq, uint32_t query_len,
                   uint32_t k, uint32_t nprobe, int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found,
                   uint64_t *n_candidates, uint32_t *nprobe_used);
int pqv_topk_depth_device(const pqv_searcher *searcher, const pqv_probe_depth *depth, const void *d_queries, uint32_t nq, uint32_t k,
                          uint32_t nprobe, int metric, int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found,
                          void *d_n_candidates, void *d_nprobe_used, void *d_tie_flags, void *hip_stream);

/* Key partitions: exact per-key top-k over a key's own rows.  The keyed, filtered and expanding calls above answer a per-query
 * filter THROUGH the IVF lists: approximate (only the probed lists are seen), at a cost that follows the probed lists' length.  For
 * many small tenants that is the wrong end of the trade.  A key partition is a second set of lists over the same rows, keyed by the
 * filter column instead of the centroids: a posting list per key value.  Nothing is probed, and the cost follows the rows that pass.
 *
 * A pqv_key_partition is made for ONE plain searcher from an integer pqv_column (PQV_COL_I32 / PQV_COL_I64, optional validity), as a
 * pqv_row_keys is.  It holds, all on the device: the searcher's list positions whose row has a valid (non-NULL) key, sorted by (key
 * as i64 ascending, row id ascending) -- an I32 column is widened, never truncated --, the distinct values ascending and the offsets
 * of each value's run.  Rows in no list (those pqv_index_remove took out) are not in it, as masks ignore them.  Positions are stored,
 * so one partition serves both layouts, a released row-order copy and the cosine layout.  pqv_key_partition_create runs on hip_stream
 * (NULL: the searcher's) and is complete on return; nothing of size O(n_rows) crosses PCIe; the result is immutable, usable from any
 * thread, and may be freed before or after its searcher.  _rows: m, the indexed rows with a valid key; _n_keys: the distinct values
 * among them; _keys: a host download for planners and tests, the first min(n, n_keys) distinct values ascending and their row counts
 * (either array may be NULL).
 * Errors of _create, in this order, NULL checks before any device use: pqv_row_keys_create's texts ("out must not be NULL", "searcher
 * must not be NULL", "column must not be NULL", "key column must be PQV_COL_I32 or PQV_COL_I64", "column has N rows, the corpus has
 * M", "column is on device D, the searcher on device E"); PQV_ERR_UNSUPPORTED "pqv_key_partition_create does not take table
 * searchers" (behind the NULL checks).
 *
 * pqv_topk_partition / pqv_topk_partition_device: no nprobe and no max_candidates.  F_q is the test of `filter` for query q
 * (PQV_KEY_EQ, PQV_KEY_RANGE, PQV_KEY_IN), read exactly as pqv_topk_filtered* reads it: host arrays in the host form; in the device
 * form device arrays read on hip_stream inside the enqueued work.
 *   candidates   query q's sequence is every partition row r with F_q(key[r]), ordered by (key[r], r): ONE contiguous span of the
 *                partition for EQ and RANGE, up to PQV_KEY_SET_MAX spans in the slice's ascending order for IN.  A candidate's
 *                position is its index in that sequence; n_candidates[q] is the sequence's length, taken before the mask.
 *   considered   the candidates the optional shared `mask` allows (NULL: all), at their unmasked positions; a row the mask excludes
 *                is never loaded.
 *   result       the k considered rows with the smallest (distance key, position), ascending.  The distance is bit for bit that of
 *                the metric's chain: PQV_L2SQ_REF4, PQV_L2SQ_SEQ, PQV_COSINE (through the cosine layout, with the halving) and
 *                PQV_DOT (ord() keys, dist = 0.0f - s(q, x)); sqrt_out as in pqv_topk.  There is no reference heap to replay and
 *                there are no tie flags: the host and the device form return the same thing.  Slots past n_found[q] hold
 *                0xFFFFFFFF / +inf.  NaN follows the key's bit order, unpinned, as everywhere.
 *   exactness    with mask == NULL the result is the exact top-k over ALL indexed rows whose key passes.  No searcher option
 *                changes a result (partition_blocks fixes the blocks per query, 0 = by rule).
 *   equivalence  let S1 be a searcher over pqv_index_from_parts(dim, 1, any centroid, one list = all indexed rows ascending) on the
 *                same corpus.  For PQV_KEY_EQ the call returns rows, distances and n_found bit for bit equal to
 *                pqv_topk_filtered_device on S1 with nprobe = 1 and max_candidates = 0; for RANGE and IN the same holds whenever no two
 *                considered rows of DIFFERENT keys tie in distance at or inside the k-th place; for PQV_DOT (which the keyed calls
 *                refuse) the twin is pqv_topk_masked_device on S1, per query under the mask M_q.
 *   counts       queries advances by nq, candidate_rows by the sum of n_candidates, embeddings_fetched by the considered rows;
 *                screened_pairs and screen_survivors do not move.
 *   limits       k <= 1024 in both forms (PQV_ERR_UNSUPPORTED "pqv_topk_partition takes k <= 1024"): there is no host fallback.
 *                n_found, n_candidates and their device forms may be NULL.  The device form is asynchronous on hip_stream with no
 *                host synchronisation; for an unvalidated IN slice that query's result is unspecified and every access is in
 *                bounds, as pqv_topk_filtered_device documents.
 *   out of scope table searchers; k > 1024 (distinct and grouped: pqv_topk_partition_grouped below; every row within a radius:
 *                pqv_range_search_partition below);
 *                mutable partitions (after an append or a remove, make the new searcher's partition); the screened kernels on long
 *                runs; choosing between the IVF and the partition path automatically (pqv_key_partition_keys gives a planner the run
 *                lengths for that choice).
 * Errors, in this order (PQV_ERR_INVALID): "searcher must not be NULL", "key partition must not be NULL", "filter must not be
 * NULL", the descriptor checks of pqv_topk_filtered (host form), "k must be > 0", "key partition belongs to another searcher", "row
 * mask belongs to another searcher", then pqv_topk's own (query length, metric).
 *
 * pqv_topk_partition_grouped / pqv_topk_partition_grouped_device: "the k nearest documents of tenant T, group_size chunks each" --
 * pqv_topk_grouped's result over pqv_topk_partition's candidates.  `group_keys` is a pqv_row_keys of this searcher (I32 or I64,
 * optional validity): the group column.  group_size == 1 is the distinct call: one pass, outputs [nq, k]; there is no separate
 * _distinct symbol, as pqv_topk_grouped has none for it either.
 *   candidates   exactly pqv_topk_partition's sequence for `filter` (EQ and RANGE: one span; IN: up to PQV_KEY_SET_MAX spans in the
 *                slice's ascending order); a candidate's position is its index in that sequence; n_candidates[q] is the sequence's
 *                length, taken before the mask and the group validity.  Host filter arrays in the host form; device arrays read on
 *                hip_stream in the device form, with pqv_topk_partition_device's unspecified-but-in-bounds rule for an unvalidated
 *                IN slice.
 *   considered   the candidates `mask` allows (NULL: all) AND whose group_keys value is valid, at their unmasked positions.  A row
 *                that fails either test is never loaded; a NULL-group row belongs to no group.
 *   result       as pqv_topk_grouped: let S be the considered rows sorted by (distance key, position).  Groups are compared in i64
 *                and ranked by their first row in S; the first k groups are kept, each with its first min(group_size, rows it has)
 *                rows in S order.  No heap replay, no tie flags: the host and the device form return the same thing.
 *   outputs      as pqv_topk_grouped: row_idx / dist [nq, k, group_size], group_key [nq, k], group_rows [nq, k], n_found [nq] (the
 *                groups found) and n_candidates [nq]; padding 0xFFFFFFFF / +inf / key 0 / count 0.  Everything but row_idx and
 *                dist may be NULL.  sqrt_out and the cosine halving as in pqv_topk_partition.
 *   metrics      PQV_L2SQ_REF4, PQV_L2SQ_SEQ, and PQV_COSINE through the cosine layout as pqv_topk_partition does it.  PQV_DOT:
 *                PQV_ERR_UNSUPPORTED "PQV_DOT is not supported by keyed and distinct calls" (the distinct lists and folds carry
 *                L2 keys).
 *   equivalence  1. on S1 (above), with row keys made from the same two columns on S1: for PQV_KEY_EQ the call equals
 *                pqv_topk_grouped_filtered_device on S1 with nprobe = 1 and max_candidates = 0, n_candidates excepted, bit for bit;
 *                for RANGE and IN the same holds whenever no two considered rows of different filter keys tie in distance.
 *                2. with every group value distinct and valid, slot i = 0 holds pqv_topk_partition_device's rows, distances and
 *                n_found, and group_rows is 1 there.  3. group_size == 1 against group_size == m: the [.., 0] slots, group_key and
 *                n_found agree.
 *   exactness    with mask == NULL the answer is exact over ALL indexed rows whose filter key passes.  No searcher option changes a
 *                result; partition_blocks fixes the blocks per query of both passes.
 *   counts       queries advances by nq, once per call (not per pass); candidate_rows by the sum of n_candidates, once;
 *                embeddings_fetched by the considered rows plus, for group_size > 1, the rows pass 2 evaluates: the considered rows
 *                of the selected groups.  screened_pairs and screen_survivors do not move.
 *   limits       k * group_size <= 1024 (the product taken in 64 bits) in both forms: PQV_ERR_UNSUPPORTED
 *                "pqv_topk_partition_grouped takes k * group_size <= 1024"; there is no host fallback.  The device form is
 *                asynchronous on hip_stream with no host synchronisation.
 *   out of scope table searchers (pqv_key_partition_create refuses them); PQV_DOT; max_nprobe (nothing is probed); the path-taking
 *                builders; choosing between the IVF and the partition path automatically.
 * Errors, in this order (PQV_ERR_INVALID), every NULL and zero check before a handle is dereferenced or a device used: "searcher
 * must not be NULL", "key partition must not be NULL", "row keys must not be NULL", "filter must not be NULL" and the descriptor
 * checks of pqv_topk_filtered (host form), "k must be > 0", "group_size must be > 0", "key partition belongs to another searcher",
 * "row keys belong to another searcher", "row mask belongs to another searcher", then pqv_topk's own (metric, query length), then the
 * two PQV_ERR_UNSUPPORTED texts above (PQV_DOT first).
 *
 * pqv_range_search_partition: "every document of tenant T within 0.3 of this vector" -- pqv_range_search's answer over
 * pqv_topk_partition's candidates, exact because nothing is probed.  The host form only: range search has no device form anywhere,
 * the output is sized from counts.  No nprobe and no max_candidates.
 *   candidates   exactly pqv_topk_partition's: query q's sequence is every partition row r with F_q(key[r]), ordered by (key[r], r);
 *                a candidate's position is its index in that sequence; n_candidates[q] is the sequence's length, taken before the
 *                mask.  The filter arrays are host arrays, read as pqv_topk_filtered reads them.
 *   considered   the candidates the optional shared `mask` allows (NULL: all), at their unmasked positions; a row the mask excludes
 *                is never loaded.
 *   distance     exactly pqv_range_search's: the bit-identical chains of PQV_L2SQ_REF4, PQV_L2SQ_SEQ, PQV_COSINE (through the cosine
 *                layout, out = 0.5f * d2 whatever sqrt_out) and PQV_DOT (dist = 0.0f - s(q, x); sqrt_out is ignored and a hit is dist
 *                <= radius); out = sqrt_out ? sqrt(d2) (correctly rounded) : d2 for the L2 forms.
 *   hit          out <= radius, inclusive, on the output scale.  A NaN distance is never a hit; radius = +inf keeps every other
 *                considered row; a negative radius keeps none, except for PQV_DOT, whose distances are signed; a NaN radius is
 *                PQV_ERR_INVALID "radius must not be NaN".
 *   order        ascending by (distance key, sequence position): unique per query, independent of scheduling and of
 *                partition_blocks.  max_results > 0 keeps the first max_results hits in that order.
 *   exactness    with mask == NULL the answer is EVERY indexed row of the passing keys within the radius.  No searcher option
 *                changes a result.
 *   equivalence  (a) for any input, ties included: with radius = +inf, max_results = k <= 1024 and no NaN distance, query q's hits
 *                are pqv_topk_partition's first n_found[q] rows and distances, bit for bit -- both calls order by (distance key,
 *                position) and neither replays a heap.  (b) on S1 (above) the call equals pqv_range_search_masked under the per-query
 *                mask M_q (the rows whose key passes F_q, ANDed with `mask`) with nprobe = 1: always for PQV_KEY_EQ; for RANGE and IN
 *                whenever no two considered rows of different keys tie in distance.
 *   output       CSR library buffers as pqv_range_search: query q's hits are row_idx / dist [lims[q], lims[q + 1]); *lims [nq + 1]
 *                is allocated also for nq = 0; release with pqv_range_free.  n_within host [nq]: the hit count before max_results;
 *                n_candidates host [nq]; both may be NULL.
 *   counts       queries advances by nq, candidate_rows by the sum of n_candidates, embeddings_fetched by the considered rows;
 *                screened_pairs and screen_survivors do not move.  pqv_set_timing / pqv_timing_read see the distance pass as the
 *                "re-rank" (one timed call per group, below).
 *   path         per piece of at most 32768 queries: the span kernel, then the candidate counts come back to the host -- ONE
 *                synchronisation more than pqv_range_search has, because the hit segments are packed (query q's holds
 *                n_candidates[q] entries, not the longest tenant's) and the grid follows the longest sequence.  The piece runs in
 *                groups of consecutive queries whose segments (12 bytes a candidate) fit a byte budget ("partition_range_bytes", 0 =
 *                1 GiB; a query whose own segment exceeds it runs alone): per group ONE exact streaming pass, the hit counts back,
 *                pqv_range_search's sort and write-out.  A group without a candidate launches nothing.
 *   limits       none on the number of hits; a sequence holds at most 2^32 - 1 candidates.
 *   out of scope table searchers; a device form; range search over the distinct or grouped forms; a per-query radius; the screened
 *                kernels on long runs.
 * Errors, in this order (PQV_ERR_INVALID), every NULL check before a handle is read or a device used: "searcher must not be NULL",
 * "key partition must not be NULL", "filter must not be NULL" and the host descriptor checks of pqv_topk_filtered, "key partition
 * belongs to another searcher", "row mask belongs to another searcher", then pqv_range_search's own: metric, query length, "radius
 * must not be NaN", "lims/row_idx/dist must not be NULL", "queries must not be NULL". */
typedef struct pqv_key_partition pqv_key_partition;
int      pqv_key_partition_create(const pqv_searcher *searcher, const pqv_column *column, void *hip_stream, pqv_key_partition **out);
uint64_t pqv_key_partition_rows(const pqv_key_partition *part);
uint64_t pqv_key_partition_n_keys(const pqv_key_partition *part);
int      pqv_key_partition_dtype(const pqv_key_partition *part);
int      pqv_key_partition_keys(const pqv_key_partition *part, int64_t *keys, uint64_t *counts, uint64_t n);
void     pqv_key_partition_free(pqv_key_partition *part);
int pqv_topk_partition(const pqv_searcher *searcher, const pqv_key_partition *part, const pqv_key_filter *filter,
                       const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, int metric,
                       int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_partition_device(const pqv_searcher *searcher, const pqv_key_partition *part, const pqv_key_filter *filter,
                              const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k, int metric, int sqrt_out,
                              void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates, void *hip_stream);
int pqv_topk_partition_grouped(const pqv_searcher *searcher, const pqv_key_partition *part, const pqv_key_filter *filter,
                               const pqv_row_keys *group_keys, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                               uint32_t query_len, uint32_t k, uint32_t group_size, int metric, int sqrt_out,
                               uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows,
                               uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_partition_grouped_device(const pqv_searcher *searcher, const pqv_key_partition *part, const pqv_key_filter *filter,
                                      const pqv_row_keys *group_keys, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                      uint32_t k, uint32_t group_size, int metric, int sqrt_out, void *d_row_idx, void *d_dist,
                                      void *d_group_key, void *d_group_rows, void *d_n_found, void *d_n_candidates, void *hip_stream);
int pqv_range_search_partition(const pqv_searcher *searcher, const pqv_key_partition *part, const pqv_key_filter *filter,
                               const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len, float radius,
                               uint64_t max_results, int metric, int sqrt_out, uint64_t **lims, uint32_t **row_idx, float **dist,
                               uint64_t *n_within, uint64_t *n_candidates);

/* Candidate lists: "the nearest 10 of exactly THESE rows" / "the distance of each of these rows" -- the second stage of hybrid
 * retrieval, where a lexical engine, a SQL sub-query, a graph walk or a coarse pass hands over a few hundred to a few thousand row
 * ids per query, different for every query.  The rows are resident: nothing crosses the bus but the ids.
 *
 * pqv_topk_rows / pqv_topk_rows_device / pqv_score_rows / pqv_score_rows_device: no nprobe and no max_candidates.  `lims` is u64
 * [nq + 1] and need not start at 0; `cand_rows` u32 row ids.  Host arrays in the host forms; in the device forms device arrays read
 * on hip_stream inside the enqueued work.
 *   candidates   query q's sequence is cand_rows[lims[q] .. lims[q + 1]) exactly as given, in any order.  A candidate's position is
 *                its index in the slice; n_candidates[q] is the slice's length, taken before any test below.  A row listed twice
 *                is two candidates and can be returned twice.
 *   considered   the candidates whose row is in one of the searcher's lists and which the optional shared `mask` allows (NULL:
 *                all), at their unmasked positions.  A row id at or above the corpus' row count, 0xFFFFFFFF, and a row
 *                pqv_index_remove* took out are not indexed.  A candidate that is not considered is never loaded.
 *   result       top-k: the k considered candidates with the smallest (distance key, position), ascending.  The distance is bit for
 *                bit that of the metric's chain: PQV_L2SQ_REF4, PQV_L2SQ_SEQ, PQV_COSINE (through the cosine layout, with the
 *                halving) and PQV_DOT (ord() keys, dist = 0.0f - s(q, x)); sqrt_out as in pqv_topk_partition.  There is no reference
 *                heap to replay and there are no tie flags: the host and the device form return the same bytes.  Slots past
 *                n_found[q] hold 0xFFFFFFFF / +inf.  n_found and n_candidates may be NULL.
 *                scores: dist[i - lims[0]] for candidate i of cand_rows is its distance on the output scale, bit-equal to what
 *                pqv_topk_rows reports for that candidate; +inf for a candidate that is not considered.  dist holds lims[nq] -
 *                lims[0] values.
 *   equivalence  with every slice ascending and unique: on S1 (pqv_topk_partition, above) rows, distances and n_found equal
 *                pqv_topk_masked_device with nprobe = 1 under the per-query mask M_q = the slice, for every metric, whenever no two
 *                considered rows tie in distance at or inside the k-th place.  With slice q = the rows of one key of a partition,
 *                ascending, the call equals pqv_topk_partition with PQV_KEY_EQ for any input, ties included: both order by
 *                (distance key, position).
 *   exactness    no searcher option changes a result (partition_blocks fixes the blocks per query, 0 = by rule, as for the
 *                partition calls).
 *   counts       queries advances by nq, candidate_rows by the sum of the slice lengths, embeddings_fetched by the considered
 *                candidates; screened_pairs and screen_survivors do not move.
 *   row map      the calls need the way back from a row id to its list position: a u32 per corpus row (4 bytes x the corpus' row
 *                count of device memory, reported with the searcher's other buffers by pqv_searcher_footprint), built by the first
 *                candidate-list call on a searcher -- one fill and one scatter kernel -- and freed with it.  It serves every layout
 *                (flags 0, PQV_LAYOUT_ROW_ORDER, PQV_RELEASE_ROW_ORDER) and the cosine layout.
 *   limits       k <= 1024 in both top-k forms (PQV_ERR_UNSUPPORTED "pqv_topk_rows takes k <= 1024"): there is no host fallback.  A
 *                slice holds at most 2^32 - 1 candidates: the host forms refuse a longer one, the device forms read its first 2^32 -
 *                1.  An inverted slice (lims[q + 1] < lims[q]) is PQV_ERR_INVALID "lims must not decrease" in the host forms and an
 *                empty sequence in the device forms.  The device forms are asynchronous on hip_stream (NULL: the searcher's stream)
 *                with no host synchronisation -- except the first candidate-list call on a searcher, which builds the row map and
 *                waits for it, as the first cosine call builds its layout.  Every access stays in bounds whatever the arrays hold,
 *                given that the slices lie inside cand_rows: a row id indexes the map only behind a compare against its length.
 *   out of scope table searchers (PQV_ERR_UNSUPPORTED "pqv_topk_rows does not take table searchers" / "pqv_score_rows does not take
 *                table searchers", behind the NULL checks); distinct, grouped and range forms over candidate lists; the
 *                path-taking builders; the screened kernels.
 * Errors, in this order, all before any device use (PQV_ERR_INVALID unless noted): "searcher must not be NULL", "lims must not be
 * NULL", "cand_rows must not be NULL" (host forms: only where some slice is non-empty), top-k: "k must be > 0", host forms: "lims
 * must not decrease" then "a candidate list holds at most 2^32 - 1 rows", "row mask belongs to another searcher", the table refusal,
 * pqv_topk's own metric and query-length texts, "row_idx/dist must not be NULL" (scores: "dist must not be NULL"), the k limit. */
int pqv_topk_rows(const pqv_searcher *searcher, const uint64_t *lims, const uint32_t *cand_rows, const pqv_row_mask *mask,
                  const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, int metric, int sqrt_out,
                  uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_rows_device(const pqv_searcher *searcher, const void *d_lims, const void *d_cand_rows, const pqv_row_mask *mask,
                         const void *d_queries, uint32_t nq, uint32_t k, int metric, int sqrt_out,
                         void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates, void *hip_stream);
int pqv_score_rows(const pqv_searcher *searcher, const uint64_t *lims, const uint32_t *cand_rows, const pqv_row_mask *mask,
                   const float *queries, uint32_t nq, uint32_t query_len, int metric, int sqrt_out, float *dist /* [lims[nq] - lims[0]] */);
int pqv_score_rows_device(const pqv_searcher *searcher, const void *d_lims, const void *d_cand_rows, const pqv_row_mask *mask,
                          const void *d_queries, uint32_t nq, int metric, int sqrt_out, void *d_dist, void *hip_stream);

/* MMR top-k: diversity by geometry -- fetch the fetch_k nearest rows, then pick k of them by maximal marginal relevance, so that
 * five paraphrases of one passage do not fill a context window.  The rows are resident: the pairwise distances are taken on the
 * device by the metric's own chain, nothing crosses the bus but the picks.
 *
 * pqv_mmr_select / pqv_mmr_select_device: the selection stage alone, over candidates the caller has -- the [nq, n] row_idx / dist
 * outputs of ANY top-k call (keyed, partition, candidate list, expanding, per-query depth) and optionally its n_found: no queries,
 * no probing.  pqv_topk_mmr / pqv_topk_mmr_device: probe + the fetch_k nearest (under `mask` where one is given) + selection.
 *   notation     one query has n candidates at positions 0 .. n-1 with rows r_i and rel_i, their distances to the query as f32 on the
 *                call's output scale (d2, sqrt(d2) with sqrt_out, 0.5f * d2 of the normalised vectors for PQV_COSINE, 0.0f - s for
 *                PQV_DOT).  lambda in [0, 1]; om = 1.0f - lambda, one f32 subtraction.
 *   considered   a candidate whose row is in one of the searcher's lists (below the corpus' row count, not 0xFFFFFFFF, not removed:
 *                pqv_topk_rows' rule) and whose position is below n_found_in[q] (NULL: n).  A candidate that is not considered is
 *                never loaded and never picked.  A row listed twice is two candidates.
 *   pd(a, b)     the metric's chain with row a in the query's place and row b as the row, put on the output scale exactly as a
 *                query distance is: PQV_L2SQ_REF4 / PQV_L2SQ_SEQ d2, or correctly rounded sqrtf(d2) with sqrt_out; PQV_COSINE the
 *                REF4 chain over the cosine layout's normalised rows, times 0.5f; PQV_DOT 0.0f - s(a, b).
 *   selection    step t = 0, 1, ... with S_t the candidates picked so far: red_t[i] = +0.0f while S_t is empty, else the f32 minimum
 *                over s in S_t of pd(r_s, r_i) -- a running minimum that starts at +inf with the first pick and takes a value only
 *                where it compares smaller, so a NaN pd leaves it as it is (the fminf rule; pd is never -0).  score_t[i] =
 *                (lambda * rel_i) - (om * red_t[i]): two f32 products and one f32 subtraction, each rounded on its own, no FMA.
 *                The pick is the considered, not yet picked candidate with the smallest (ord(score_t[i]), i), ord() as for PQV_DOT
 *                on the score's bits: a total order, NaN and +-0 included, the lowest position winning a tie.  Selection ends after
 *                min(k, considered) picks; that count is n_found[q].
 *   outputs      in PICK order, not by distance: row_idx[q, j] the j-th pick's row, dist[q, j] its rel bit for bit, score[q, j] its
 *                score_t at the time of the pick; past n_found 0xFFFFFFFF / +inf / +inf.  score and n_found may be NULL.
 *   lambda       1: om is +0.0f and for finite rel the picks are the first k considered candidates by (ord(rel), i) -- with
 *                candidates in ascending rel, the input order.  The first pick is always the considered candidate with the smallest
 *                (ord(lambda * rel), i).
 *   stage 1      of pqv_topk_mmr*: exactly pqv_topk_device with k = fetch_k, or pqv_topk_masked_device where mask is not NULL, on
 *                whatever route the searcher's dispatch picks, the screened kernels included; its result is in (d2, position) order
 *                -- in both forms no reference heap is replayed and there are no tie flags -- and stays in the call's scratch lane,
 *                the selection running over it on the same stream.  n_candidates is stage 1's.  The fused call equals
 *                pqv_mmr_select_device over the outputs of that stage-1 call, bit for bit.
 *   exactness    no searcher option changes a result.
 *   counts       as for the stage-1 call of the same shape; pqv_mmr_select* advances queries by nq.  The selection itself moves
 *                kernel_launches only.
 *   limits       n, fetch_k <= 1024 and at most 1024 probed lists per query (PQV_ERR_UNSUPPORTED): there is no host fallback.
 *                PQV_DOT keeps its own limits.  The device forms are asynchronous on hip_stream (NULL: the searcher's stream) with
 *                no host synchronisation -- except the first call on a searcher that needs the row map (pqv_topk_rows: row map),
 *                and the first cosine call.  Every access stays in bounds whatever cand_rows holds: a row id indexes the map only
 *                behind a compare against its length.
 *   work         (picks - 1) x considered row reads per query, served from the caches behind the first pass.
 *   out of scope table searchers; keyed, distinct and grouped stage 1 inside the fused call (pqv_mmr_select* takes their outputs);
 *                n above 1024; a screened redundancy pass.
 * Errors, in this order, all before any device use (PQV_ERR_INVALID unless noted): "searcher must not be NULL", "k must be > 0",
 * fused: "fetch_k must be >= k" (n < k is fine for the selection: fewer picks), "lambda must be in [0, 1]" (a NaN too),
 * PQV_ERR_UNSUPPORTED "pqv_topk_mmr takes fetch_k <= 1024" / "pqv_mmr_select takes n <= 1024", "row mask belongs to another
 * searcher", PQV_ERR_UNSUPPORTED "pqv_topk_mmr does not take table searchers" / "pqv_mmr_select does not take table searchers",
 * pqv_topk's own nprobe and metric texts, PQV_DOT's limits, PQV_ERR_UNSUPPORTED "pqv_topk_mmr takes min(nprobe, n_clusters) <= 1024",
 * the query-length text, then the NULL pointers ("cand_rows/cand_dist must not be NULL", "row_idx/dist must not be NULL"). */
int pqv_mmr_select(const pqv_searcher *searcher, const uint32_t *cand_rows /* [nq, n] */, const float *cand_dist /* [nq, n] */,
                   const uint32_t *n_found_in /* [nq], may be NULL: n for every query */, uint32_t nq, uint32_t n, uint32_t k,
                   float lambda, int metric, int sqrt_out, uint32_t *row_idx, float *dist, float *score, uint32_t *n_found);
int pqv_mmr_select_device(const pqv_searcher *searcher, const void *d_cand_rows, const void *d_cand_dist, const void *d_n_found_in,
                          uint32_t nq, uint32_t n, uint32_t k, float lambda, int metric, int sqrt_out, void *d_row_idx, void *d_dist,
                          void *d_score, void *d_n_found, void *hip_stream);
int pqv_topk_mmr(const pqv_searcher *searcher, const pqv_row_mask *mask /* may be NULL */, const float *queries, uint32_t nq,
                 uint32_t query_len, uint32_t k, uint32_t fetch_k, float lambda, uint32_t nprobe, uint64_t max_candidates, int metric,
                 int sqrt_out, uint32_t *row_idx, float *dist, float *score, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_mmr_device(const pqv_searcher *searcher, const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k,
                        uint32_t fetch_k, float lambda, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                        void *d_row_idx, void *d_dist, void *d_score, void *d_n_found, void *d_n_candidates, void *hip_stream);

/* Distinct top-k: the nearest row of each of the k nearest GROUPS -- `SELECT DISTINCT ON (doc_id) .. ORDER BY array_distance(col, q)
 * LIMIT k` over chunked embeddings (several rows per document, product, user); elsewhere called grouping or collapse.
 *
 * A distinct call is the masked call of the same arguments plus a group column `keys`: a pqv_row_keys of this searcher (I32 or
 * I64, optional validity).  `mask` is an optional shared row mask, NULL: none.
 *   considered rows  the unmasked candidate sequence, cut by max_candidates / a table's round-robin quotas BEFORE any filter; of
 *                    the capped candidates, those whose key is valid (not NULL) and which the mask allows, at their UNMASKED
 *                    positions.  A NULL-key row belongs to no group and is never returned (as a NULL row never matches a keyed call).
 *   group            all considered rows of equal key value, compared in i64 (an I32 column is widened); its representative is
 *                    its considered row with the smallest (d2, position).
 *   result           query q: the k representatives with the smallest (d2, position), ascending by that pair -- always: the
 *                    reference has no grouping, so there is no heap history to replay and there are no tie flags; the host and
 *                    the device form return the same thing.  NaN distances follow the key's bit order, as in
 *                    pqv_topk_masked_device (unpinned, as everywhere).
 *   outputs          row_idx, dist and group_key (int64_t [nq * k]: the representatives' key values), n_found (groups found, at
 *                    most k) and n_candidates; entries past n_found[q] are 0xFFFFFFFF, +inf and 0.  sqrt_out and the PQV_COSINE
 *                    halving are the masked call's.  group_key / d_group_key, n_found and n_candidates may be NULL.
 *   counts           n_candidates and candidate_rows are the counts before cap and filter; embeddings_fetched advances by the
 *                    considered rows.
 *   equivalence      query q's result is the (d2, position)-sorted sequence of its considered rows with only the FIRST row of
 *                    every key value kept, cut to k; that sorted sequence is what pqv_range_search_masked returns with radius =
 *                    +inf, sqrt_out = 0 and the same mask ANDed with the key validity.  Hence with all keys distinct the call
 *                    returns, bit for bit, what pqv_topk_masked_device returns (rows, distances, n_found).
 *   path             always the exact streaming pass with lists that hold at most one entry per group: no searcher option
 *                    changes a result, and excluded rows are never read.  Plain and table searchers, every layout, PQV_COSINE
 *                    through the cosine layout.  The kernels serve k <= 1024 and at most 1024 probed lists; beyond that
 *                    pqv_topk_distinct computes the sorted considered sequence with the masked range machinery (radius = +inf)
 *                    and keeps the first row per key on the host, and pqv_topk_distinct_device reports PQV_ERR_UNSUPPORTED, as
 *                    pqv_topk_masked_device does.
 *   out of scope     distinct range search.  (A per-query key filter together with the group column: pqv_topk_distinct_filtered
 *                    below.  More than one row per group: pqv_topk_grouped below.)
 * Errors (PQV_ERR_INVALID; NULL handles are checked before any device use): "searcher must not be NULL", "row keys must not be
 * NULL", "row keys belong to another searcher", "row mask belongs to another searcher", and pqv_topk's own ("k must be > 0", ...). */
int pqv_topk_distinct(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_row_mask *mask, const float *queries,
                      uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric,
                      int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_distinct_device(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_row_mask *mask,
                             const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric,
                             int sqrt_out, void *d_row_idx, void *d_dist, void *d_group_key, void *d_n_found,
                             void *d_n_candidates, void *hip_stream);

/* Grouped top-k: up to group_size rows of each of the k nearest GROUPS -- "the 10 nearest documents and the 3 best chunks of each";
 * `ROW_NUMBER() OVER (PARTITION BY doc_id ORDER BY distance) <= group_size` on the k nearest doc_ids; elsewhere search_groups,
 * group_by_field + group_size, collapse + inner_hits.
 *
 * A grouped call is the distinct call of the same arguments plus group_size.  Considered rows, groups and representatives are
 * exactly pqv_topk_distinct's: the cap cuts the candidate sequence before any filter, a row is considered when its key is valid
 * and the optional shared mask allows it, positions are the unmasked ones, keys are compared in i64.
 *   result           let S be query q's considered rows sorted by (d2, position).  Groups are ranked by their first row in S and
 *                    the first k groups are kept; group g returns its first min(group_size, rows it has in S) rows, in S order.
 *                    No heap to replay and no tie flags: the host and the device form return the same thing.
 *   outputs          row_idx and dist [nq, k, group_size]: group g's i-th row at [q][g][i]; group_key (int64_t [nq, k]): the
 *                    group's key value; group_rows (uint32_t [nq, k]): the rows returned for the group; n_found [nq]: the groups
 *                    found, at most k; n_candidates.  Empty row slots hold 0xFFFFFFFF / +inf, empty group slots key 0 and count
 *                    0.  sqrt_out and the PQV_COSINE halving are the distinct call's.  group_key, group_rows, n_found and
 *                    n_candidates (and their d_ forms) may be NULL.
 *   equivalence      each bit for bit: group_size == 1 returns what pqv_topk_distinct returns and takes that path unchanged (one
 *                    pass); with all keys distinct, slot i = 0 holds pqv_topk_masked_device's result; in general S is what
 *                    pqv_range_search_masked returns with radius = +inf, sqrt_out = 0 and the mask ANDed with the key validity.
 *   path             group_size > 1 is two exact streaming passes over the same candidates: the distinct pass names the k groups,
 *                    the second pass reads only the rows of those groups and keeps at most group_size per group.  No searcher
 *                    option changes a result.  The kernels serve k * group_size <= 1024 (computed in 64 bits) and at most 1024
 *                    probed lists; beyond that pqv_topk_grouped computes S with the masked range machinery and groups on the
 *                    host, and pqv_topk_grouped_device reports PQV_ERR_UNSUPPORTED "pqv_topk_grouped_device takes k *
 *                    group_size <= 1024 and at most 1024 probed lists per query".
 *   counts           group_size > 1: queries and candidate_rows advance once per query, not once per pass; embeddings_fetched
 *                    advances by the considered rows plus the rows the second pass evaluates, the considered rows of the selected
 *                    groups.  group_size == 1: the distinct call's counts.
 *   out of scope     grouped range search; PQV_DOT.  (A per-query key filter together with grouping: pqv_topk_grouped_filtered
 *                    below.  Probing further lists when fewer than k groups are found: pqv_topk_grouped_expand below.)
 * Errors: pqv_topk_distinct's, in the same order, NULL handles checked before any device use; behind "k must be > 0":
 * "group_size must be > 0".  PQV_DOT: PQV_ERR_UNSUPPORTED "PQV_DOT is not supported by keyed and distinct calls". */
int pqv_topk_grouped(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_row_mask *mask, const float *queries,
                     uint32_t nq, uint32_t query_len, uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates,
                     int metric, int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows,
                     uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_grouped_device(const pqv_searcher *searcher, const pqv_row_keys *keys, const pqv_row_mask *mask, const void *d_queries,
                            uint32_t nq, uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates, int metric,
                            int sqrt_out, void *d_row_idx, void *d_dist, void *d_group_key, void *d_group_rows, void *d_n_found,
                            void *d_n_candidates, void *hip_stream);

/* Distinct and grouped top-k under a PER-QUERY key filter: every query of a batch has its own `tenant = ?`, `group_id IN (...)`
 * or `ts BETWEEN ? AND ?` and gets the k nearest DOCUMENTS back -- multi-tenant retrieval over chunked documents in one call.
 *
 * Each call is its twin (pqv_topk_distinct*, pqv_topk_grouped*) with `filter_keys, filter` behind the group column `group_keys`:
 * filter_keys is a second pqv_row_keys of this searcher (it may be the same object as group_keys) and filter the descriptor of
 * pqv_topk_filtered, read as that call reads it -- host arrays in the host forms; in the device forms DEVICE arrays read on
 * hip_stream inside the enqueued work, the calls stay asynchronous, and an unvalidated PQV_KEY_IN slice has the unspecified but
 * in-bounds behaviour pqv_topk_filtered_device documents.  `mask` is an optional shared row mask, NULL: none.
 *   contract         let F_q be the descriptor's test for query q, exactly as pqv_topk_filtered defines it, and
 *                      M_q[r] = filter_valid[r] && F_q((int64_t) filter_column[r]) && (mask ? mask[r] : 1).
 *                    Query q returns, bit for bit, what pqv_topk_distinct / pqv_topk_grouped returns for that one query with the
 *                    shared mask M_q: rows, distances, group keys, group_rows, n_found and n_candidates.
 *   the twin's       everything else, word for word: the cap cuts the candidate sequence BEFORE any filter and positions stay the
 *                    unmasked ones; a row is considered iff M_q holds AND its group key is valid; groups are compared in i64; the
 *                    order is (d2, position) always -- no heap replay, no tie flags; sqrt_out and the PQV_COSINE halving;
 *                    group_size == 1 is the distinct call; the counters (embeddings_fetched advances by the considered rows summed
 *                    over the batch, plus the second pass's rows of a grouped call).  Plain and table searchers, every layout,
 *                    PQV_L2SQ_REF4 / PQV_L2SQ_SEQ / PQV_COSINE.
 *   consequences     the filter applies BEFORE the representative is chosen: a group whose nearest row fails F_q is represented by
 *                    its nearest PASSING row, or absent if none passes.  PQV_KEY_RANGE over [INT64_MIN, INT64_MAX] on a column
 *                    without NULLs is the unfiltered twin.  With all group keys distinct, slot 0 holds pqv_topk_filtered_device's
 *                    result.
 *   path             the twins' exact streaming passes, a window's positions also tested against the query's filter: a row the
 *                    filter excludes is never read.  Beyond the kernels' lists (k * group_size > 1024, or more than 1024 probed
 *                    lists) the host forms compute the sorted considered sequence with the filtered range machinery (radius =
 *                    +inf, the group validity AND the shared mask as the image, the per-query filter beside it) and group on the
 *                    host; the device forms report the twins' PQV_ERR_UNSUPPORTED.
 *   out of scope     PQV_DOT: PQV_ERR_UNSUPPORTED "PQV_DOT is not supported by keyed and distinct calls".  (Expansion (max_nprobe)
 *                    with a group column: pqv_topk_distinct_expand below.)
 * Errors (PQV_ERR_INVALID), in this order, every NULL and zero check before a handle is dereferenced or a device used: "searcher
 * must not be NULL", "row keys must not be NULL" (group_keys), "a key filter needs row keys" (filter_keys), "filter must not be
 * NULL", the descriptor checks of pqv_topk_filtered, "k must be > 0", "group_size must be > 0" (grouped), "row keys belong to
 * another searcher" (either column), "row mask belongs to another searcher", and the rest of pqv_topk's. */
int pqv_topk_distinct_filtered(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                               const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                               uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                               uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_distinct_filtered_device(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                      const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                      uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                      void *d_row_idx, void *d_dist, void *d_group_key, void *d_n_found, void *d_n_candidates,
                                      void *hip_stream);
int pqv_topk_grouped_filtered(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                              const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                              uint32_t query_len, uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates,
                              int metric, int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows,
                              uint32_t *n_found, uint64_t *n_candidates);
int pqv_topk_grouped_filtered_device(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                     const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                     uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates, int metric,
                                     int sqrt_out, void *d_row_idx, void *d_dist, void *d_group_key, void *d_group_rows,
                                     void *d_n_found, void *d_n_candidates, void *hip_stream);

/* Expanding distinct and grouped top-k: every query probes on until k GROUPS are found -- the k nearest documents of a tenant
 * without raising nprobe for the whole batch and without a round trip per short query.
 *
 * Each call is its twin with max_nprobe where max_candidates stands and one more output, nprobe_used (uint32_t [nq]).  The twin is
 * chosen by the filter arguments: filter_keys == NULL && filter == NULL -- pqv_topk_distinct / pqv_topk_grouped (`mask` optional, so
 * a plain distinct call expands too); both non-NULL -- pqv_topk_distinct_filtered / pqv_topk_grouped_filtered.
 *   rule       kc lists, p0 = min(nprobe, kc), P = min(max_nprobe, kc); M_q the twin's row set of query q (the shared mask, ANDed
 *              with the filter column's validity and the query's test in the filtered forms).  gcnt_q(p) = the DISTINCT i64 group
 *              values among the rows r of the first p lists of q's probe order whose group key is valid and for which M_q[r]
 *              holds -- whatever their distance, nothing capped.  nprobe_used[q] = the smallest p in [p0, P] with gcnt_q(p) >= k,
 *              P where there is none.  group_size plays no part: the target is k groups.
 *   result     query q returns, bit for bit, what the twin returns for that one query with nprobe = nprobe_used[q] and
 *              max_candidates = 0: row_idx, dist, group_key, group_rows (grouped) and n_found; n_candidates[q] is the summed
 *              length of the used lists.  The counters advance as for those nq twin calls; the counting pass reads no embedding
 *              and counts nothing.  No new result is defined: the probe order is prefix-consistent and positions are prefix sums
 *              in it, as for pqv_topk_expand.  No tie flags and no heap replay, as the twins; the host and the device form
 *              return the same thing.  max_nprobe == nprobe is the twin call itself.
 *   scope      plain searchers, both layouts, PQV_L2SQ_REF4 / PQV_L2SQ_SEQ / PQV_COSINE (through the cosine layout, as the twins),
 *              I32 and I64 group columns with or without validity, all three filter kinds.  Every output except row_idx and
 *              dist may be NULL.  The device forms are asynchronous on hip_stream with no host synchronisation; device filter
 *              arrays are read inside the enqueued work.
 *   path       the probe ranks P lists per query; ONE counting kernel (a block per query) walks the lists in probe order over
 *              the stream passes' own windows and keeps the group values seen in an exact hash set until it holds k; the twin's
 *              stream pass or passes then walk each query's lists below its own limit, and the twin's merge follows.
 *   out of scope  table searchers, PQV_DOT, max_candidates, range search, and -- for the host forms too -- lists beyond the kernels'.
 * Errors (PQV_ERR_INVALID), in this order, every NULL and zero check before a handle is read: "searcher must not be NULL", "row
 * keys must not be NULL" (group_keys), "a key filter needs row keys" (filter without filter_keys), "filter must not be NULL"
 * (filter_keys without filter), the descriptor checks of pqv_topk_filtered, "max_nprobe must be >= nprobe", "k must be > 0",
 * "group_size must be > 0" (grouped), "row keys belong to another searcher" (either column), "row mask belongs to another
 * searcher", and the rest of pqv_topk's.  PQV_ERR_UNSUPPORTED, both forms: "pqv_topk_distinct_expand does not take table searchers"
 * (grouped: its own name), "PQV_DOT is not supported by keyed and distinct calls", "pqv_topk_distinct_expand takes k <= 1024 and
 * at most 1024 probed lists per query", "pqv_topk_grouped_expand takes k * group_size <= 1024 and at most 1024 probed lists per
 * query" (the product in 64 bits; the host forms do not fall back to the range machinery). */
int pqv_topk_distinct_expand(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                             const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                             uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t max_nprobe, int metric, int sqrt_out,
                             uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *n_found, uint64_t *n_candidates,
                             uint32_t *nprobe_used);
int pqv_topk_distinct_expand_device(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                    const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                    uint32_t k, uint32_t nprobe, uint32_t max_nprobe, int metric, int sqrt_out, void *d_row_idx,
                                    void *d_dist, void *d_group_key, void *d_n_found, void *d_n_candidates, void *d_nprobe_used,
                                    void *hip_stream);
int pqv_topk_grouped_expand(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                            const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                            uint32_t query_len, uint32_t k, uint32_t group_size, uint32_t nprobe, uint32_t max_nprobe, int metric,
                            int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows,
                            uint32_t *n_found, uint64_t *n_candidates, uint32_t *nprobe_used);
int pqv_topk_grouped_expand_device(const pqv_searcher *searcher, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                   const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                   uint32_t k, uint32_t group_size, uint32_t nprobe, uint32_t max_nprobe, int metric, int sqrt_out,
                                   void *d_row_idx, void *d_dist, void *d_group_key, void *d_group_rows, void *d_n_found,
                                   void *d_n_candidates, void *d_nprobe_used, void *hip_stream);

/* Exhaustive top-k of nq queries over EVERY row of the resident column (no index), batched
 * on the matrix cores: what DataFusion's brute-force `ORDER BY array_distance(..) LIMIT k`
 * baseline does row by row (benches/query.rs:76-98), for the metrics above.  Results are
 * ordered ascending by (distance, row id).  Host arrays as in pqv_topk. */
int pqv_brute_topk(const pqv_corpus *corpus, const float *queries, uint32_t nq, uint32_t query_len,
                   uint32_t k, int metric, uint32_t *row_idx, float *dist, uint32_t *n_found);

/* update_topk_heap / compute_distance_values (src/df_vector/exec.rs:457-550) for one RecordBatch worth of rows:
 * cand host [m, dim] values buffer, ids[m] the payload to return (e.g. batch row numbers; NULL => 0..m), valid[m]
 * optional bytes (0 = null row or length mismatch => skipped, exec.rs:496-498,526-528).  The batch's distances are
 * computed on the GPU in compute_distance_values' order; the rows then pass through the reference's heap policy --
 * std's BinaryHeap push / peek / pop, restated exactly -- in arrival order, so results equal the reference's in every
 * non-NaN case, ties included.  The running state io_rows / io_d2 / io_count (caller-owned, capacity k) IS that heap's
 * backing array between batches (NOT sorted); pass *io_count = 0 for the first batch and call pqv_rerank_finish after
 * the last.  Any k > 0 (the selection is the heap's; no kernel-side list).
 * pqv_rerank_f64: the same for a Float64 values buffer, each value narrowed `as f32` first (exec.rs:538-545).
 * pqv_rerank_finish: heap.into_iter() + the stable sort by distance of exec.rs:269-274 -> out_rows / out_d2 [count]
 * ascending (host-only; the DataFusion path emits no distance column and takes no sqrt). */
int pqv_rerank(int device, const float *query, const float *cand, const uint32_t *ids,
               const uint8_t *valid, uint64_t m, uint32_t dim, uint32_t k, int metric,
               uint32_t *io_rows, float *io_d2, uint32_t *io_count);
int pqv_rerank_f64(int device, const float *query, const double *cand, const uint32_t *ids,
                   const uint8_t *valid, uint64_t m, uint32_t dim, uint32_t k, int metric,
                   uint32_t *io_rows, float *io_d2, uint32_t *io_count);
int pqv_rerank_finish(const uint32_t *io_rows, const float *io_d2, uint32_t count, uint32_t *out_rows, float *out_d2);

/* The same fold for a batch that is ALREADY resident on `device` (e.g. a decoded Arrow values buffer uploaded by the
 * scan): d_cand [m, dim] f32, d_ids u32[m] or NULL (=> 0..m), the running state d_io_rows u32[k] / d_io_d2 f32[k] /
 * d_io_count u32[1] lives on the device between batches, kept SORTED ascending by (d2, arrival) -- a different state
 * form from pqv_rerank's heap array; do not mix the two on one state (a device count above k is read as k).  No null
 * mask (compact before the call).  k <= 1024.  Enqueued on hip_stream (NULL: a library stream) and completed before
 * the call returns.  Everything stays on the GPU, so the heap's sift history is not replayed: the result is the k
 * smallest by (d2, arrival), equal to the reference's whenever no two of the k results (nor the k-th and the first
 * excluded row) have the same distance.
 * pqv_rerank_device_flags also maintains d_tie_flag (device u32[1], zeroed by the caller before the first batch,
 * sticky): set when such a tie was seen in any fold so far -- then, and only then, the reference's survivors / order
 * may differ and the caller re-runs those batches through pqv_rerank (k <= 1023: the lists carry a runner-up). */
int pqv_rerank_device(int device, const void *d_query, const void *d_cand, const void *d_ids, uint64_t m, uint32_t dim,
                      uint32_t k, int metric, void *d_io_rows, void *d_io_d2, void *d_io_count, void *hip_stream);
int pqv_rerank_device_flags(int device, const void *d_query, const void *d_cand, const void *d_ids, uint64_t m, uint32_t dim,
                            uint32_t k, int metric, void *d_io_rows, void *d_io_d2, void *d_io_count, void *d_tie_flag,
                            void *hip_stream);

/* Merge per-shard top-k lists (one list per file/shard, as topk_from_batches does for
 * multi-file tables, src/df_vector/exec.rs:264-267): lists [n_lists, nq, k] of d2 (or
 * distance) and row ids, counts [n_lists, nq]; ties resolve by (value, list index,
 * position in list).  Host arrays. out_list receives the source list of each result. */
int pqv_merge_topk(const float *dist, const uint32_t *rows, const uint32_t *counts,
                   uint32_t n_lists, uint32_t nq, uint32_t k, float *out_dist,
                   uint32_t *out_rows, uint32_t *out_list, uint32_t *out_count);

/* Device-resident form of the merge for the multi-GPU exchange: d_dist f32 / d_rows u32
 * [n_lists, nq, k] as delivered by one all-gather of every rank's pqv_topk_device outputs
 * (empty slots: 0xFFFFFFFF rows), d_row_base i64[n_lists] the first global row of each shard.
 * Writes d_out_dist f32[nq, k] and d_out_rows i64[nq, k] (global row ids, -1 = none), ordered
 * by (distance, list, position).  Asynchronous on hip_stream (NULL = the default stream). */
int pqv_merge_topk_device(int device, const void *d_dist, const void *d_rows, const void *d_row_base,
                          uint32_t n_lists, uint32_t nq, uint32_t k, void *d_out_dist,
                          void *d_out_rows, void *hip_stream);

/* The same merge over PACKED lists: d_pairs [n_lists, nq, k] of {f32 distance, u32 row} (8 bytes per result), the
 * form in which ONE all-gather delivers every rank's top-k (pq_vector_amd/sharding.py). */
int pqv_merge_topk_packed_device(int device, const void *d_pairs, const void *d_row_base, uint32_t n_lists,
                                 uint32_t nq, uint32_t k, void *d_out_dist, void *d_out_rows, void *hip_stream);

/* ---- the exchange itself, without torch --------------------------------------------------------------------------
 * Multi-file tables are probed file by file and merged in ONE heap (src/df_vector/index_exec.rs:85-164,
 * src/df_vector/exec.rs:264-267).  With one shard (file / row-group range) per GPU that heap is one RCCL all-gather of
 * every rank's k packed {distance, row} results per query over xGMI followed by the merge above on every rank.  These
 * entry points let the Rust host do that with nothing but this library: librccl is resolved at run time (a copy the
 * process already loaded -- same SONAME -- else the loader path, else /opt/rocm/lib; PQV_RCCL_LIB overrides) and is
 * only needed by these calls.
 *   unique_id     rank 0 draws the 128-byte rendezvous id (ncclGetUniqueId) and hands it to every rank over the host's
 *                 own channel (a file, a socket, the DataFusion coordinator)
 *   comm_create   collective over all `world` ranks (ncclCommInitRank), one process per GPU
 *   comm_adopt    wraps an existing ncclComm_t (passed as void*) of THE SAME librccl (pqv_shard_rccl_path says which
 *                 one this library bound); the caller keeps ownership of it
 *   exchange      d_dist f32 / d_rows u32 [nq, k]: this rank's pqv_topk_device outputs (empty slots 0xFFFFFFFF);
 *                 d_row_base i64[world]: first global row of every shard; writes d_out_dist f32 / d_out_rows i64 [nq, k]
 *                 ordered by (distance, shard, position) -- identical on every rank.  Asynchronous on hip_stream; calls
 *                 on one communicator must not overlap (one stream, or the caller's own ordering). */
#define PQV_SHARD_ID_BYTES 128
typedef struct pqv_shard_comm pqv_shard_comm;
const char *pqv_shard_rccl_path(void);
int  pqv_shard_unique_id(uint8_t *id /* [PQV_SHARD_ID_BYTES] */);
int  pqv_shard_comm_create(int device, uint32_t rank, uint32_t world, const uint8_t *id, pqv_shard_comm **out);
int  pqv_shard_comm_adopt(int device, void *nccl_comm, pqv_shard_comm **out);
/* ONE Parquet file shared by `world` GPUs (host only; no device is touched): the half-open row-group range [*rg_lo, *rg_hi) of
 * shard `rank`, the file-global row id of its first row (*row_base = rows of the row groups before it: how the reference maps
 * file-global row ids to row groups, src/df_vector/access.rs:128-144) and its row count.  rg_rows[i] = rows of row group i in
 * file order.  Cut r (between shards r - 1 and r) is the row-group boundary whose prefix sum is nearest to r n / world -- the lower
 * one on a tie, never before the previous cut; every rank computes every cut from the footer alone, the ranges tile the file, a row
 * group is never split, and with fewer row groups than shards the surplus shards are empty (*n_rows = 0). */
int  pqv_shard_row_groups(const uint64_t *rg_rows, uint32_t n_row_groups, uint32_t rank, uint32_t world,
                          uint32_t *rg_lo, uint32_t *rg_hi, uint64_t *row_base, uint64_t *n_rows);
uint32_t pqv_shard_comm_rank(const pqv_shard_comm *comm);
uint32_t pqv_shard_comm_world(const pqv_shard_comm *comm);
int  pqv_shard_exchange(pqv_shard_comm *comm, const void *d_dist, const void *d_rows, const void *d_row_base,
                        uint32_t nq, uint32_t k, void *d_out_dist, void *d_out_rows, void *hip_stream);
void pqv_shard_comm_free(pqv_shard_comm *comm);

/* CandidateCursor (src/df_vector/access.rs:193-243; used at src/df_vector/exec.rs:224-231): when a query over a
 * multi-file table carries max_candidates, candidates are taken round-robin across the files -- one per file and
 * turn, each file's own list in probe-rank order -- until the cap; the round-robin position persists between
 * batches.  Host-side integer logic (no device needed).  A file's share of a batch is always the next PREFIX of its
 * list, so per_file_taken (optional, [file_count], cumulative) is what to pass as pqv_topk's max_candidates for
 * that file's searcher.
 *   add:        replaces file idx's candidate list (rows are copied); idx >= file_count is ignored like the reference
 *   next_batch: out_file / out_row have room for batch_size entries; *n_out receives the count */
typedef struct pqv_candidate_cursor pqv_candidate_cursor;
int  pqv_candidate_cursor_new(uint32_t file_count, pqv_candidate_cursor **out);
int  pqv_candidate_cursor_add(pqv_candidate_cursor *cursor, uint32_t idx, const uint32_t *rows, uint64_t n_rows);
int  pqv_candidate_cursor_next_batch(pqv_candidate_cursor *cursor, uint64_t batch_size, uint32_t *out_file,
                                     uint32_t *out_row, uint64_t *n_out, uint64_t *per_file_taken);
void pqv_candidate_cursor_free(pqv_candidate_cursor *cursor);

/* Counters mirroring the reference's plan metrics (src/df_vector/index_exec.rs:289-299,
 * src/df_vector/exec.rs:411-427), accumulated per searcher since creation. */
typedef struct pqv_counters_t {
    uint64_t queries;            /* top-k queries served                                 */
    uint64_t candidate_rows;     /* sum over queries of probed list lengths              */
    uint64_t embeddings_fetched; /* rows whose distance was computed (after the cap)     */
    uint64_t kernel_launches;    /* device kernels enqueued                              */
    uint64_t exact_replays;      /* pqv_topk queries replayed through the exact heap     */
    uint64_t screened_pairs;     /* (row, query) pairs put through the MFMA lower-bound   */
    uint64_t screen_survivors;   /* ... of which were evaluated exactly                   */
} pqv_counters_t;
int pqv_counters(const pqv_searcher *searcher, pqv_counters_t *out);

/* Diagnostic: the library's own restatement of rand 0.8.5's StdRng (ChaCha12) and seq::index::sample, which draw
 * every seeded choice of the index build (src/ivf/index.rs:231-232,327,337,340,373,385).  Exposed so that tests can
 * pin it to rand's published value-stability vectors and cross-check it against the CPU oracle's independent C
 * restatement.  seed32 != NULL: StdRng::from_seed(seed32), else StdRng::seed_from_u64(seed64).
 *   mode 0: out[i] = next_u64()            mode 1: out[i] = next_u32()
 *   mode 2: out[i] = gen_range(0..arg) usize                mode 3: out[i] = bits of gen_range(0.0f32..1.0)
 *   mode 4: out[0..n) = index::sample(rng, length = arg, amount = n) */
int pqv_diag_rng(const uint8_t *seed32, uint64_t seed64, int mode, uint64_t arg, uint64_t *out, uint64_t n);

/* Kernel timing for bench.py's roofline line.  While enabled, every pqv_topk /
 * pqv_topk_device call records HIP events on the stream its kernels run on: around the
 * whole call and around the re-rank kernel alone.  pqv_timing_read synchronises those
 * events, returns the summed milliseconds and the number of calls since the last read,
 * and clears them. */
int pqv_set_timing(pqv_searcher *searcher, int enabled);
int pqv_timing_read(const pqv_searcher *searcher, double *rerank_ms, double *total_ms,
                    uint32_t *n_calls);

#ifdef __cplusplus
}
#endif
#endif /* PQV_H */
