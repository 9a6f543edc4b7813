//! Safe wrappers over `libpqv_hip.so`, mirroring the types pq-vector's callers use today so that the crate's
//! public API (`IndexBuilder`, `TopkBuilder`, `SearchResult`) keeps its shape while the IVF core runs on the GPU:
//!
//! | pq-vector (reference)                                          | here                                   |
//! |-----------------------------------------------------------------|----------------------------------------|
//! | `Embeddings { data: Vec<f32>, dim }` `src/ivf/mod.rs:72-102`    | [`Corpus`] (the column, resident in HBM) |
//! | `build_ivf_index(&Embeddings, IvfBuildConfig)` `src/ivf/index.rs:152-214` | [`IndexBuilder::build`]        |
//! | `IvfIndex::{to_bytes, from_bytes, dim}` `src/ivf/index.rs:53-128` | [`Index`]                            |
//! | `IvfIndex::candidate_rows` `:57-63`                             | [`Searcher::candidate_rows`]           |
//! | `topk()` / `TopkBuilder` / `SearchResult` `src/ivf/search.rs:41-142` | [`TopkBuilder`], [`SearchResult`], [`Searcher::topk`] |
//! | `update_topk_heap` `src/df_vector/exec.rs:457-484`              | [`RerankState::fold_batch`]            |
//! | `CandidateCursor` `src/df_vector/access.rs:193-243`             | [`CandidateCursor`]                    |
//! | one heap over all files `src/df_vector/exec.rs:264-267`         | [`ShardComm::exchange`] (RCCL all-gather + merge) |
//!
//! Not compiled in the environment this repository was built in (no Rust toolchain in the image);
//! `tests/test_rust_binding.py` keeps `sys.rs` in lock-step with `include/pqv.h`, and every `sys::pqv_*` call below is
//! checked by that test to exist with the right number of arguments.  Error texts are the library's, which are the
//! reference's own (`"k must be > 0"`, `"Query dimension mismatch: expected {}, got {}"`, ...).
pub mod sys;
/// The reference's path-taking call shapes -- `IndexBuilder::new(source, column).build_inplace()`, `TopkBuilder::new(path, &query)`
/// -- over an indexed Parquet file (cargo feature `parquet-files`).
#[cfg(feature = "parquet-files")]
pub mod file;

use std::ffi::CStr;
use std::num::NonZeroUsize;
use std::os::raw::{c_int, c_void};
use std::ptr;

pub type Error = Box<dyn std::error::Error + Send + Sync>;
pub type Result<T> = std::result::Result<T, Error>;

pub(crate) fn check(rc: c_int) -> Result<()> {
    if rc == sys::PQV_OK {
        return Ok(());
    }
    // thread-local message of the failing call on THIS thread
    let msg = unsafe { CStr::from_ptr(sys::pqv_last_error()) }.to_string_lossy().into_owned();
    Err(msg.into())
}

/// Number of usable HIP devices (0 without a GPU; the library has no CPU fallback).
pub fn device_count() -> usize {
    unsafe { sys::pqv_device_count() }.max(0) as usize
}

/// The embedding column in one GPU's HBM (replaces the materialised `Embeddings`).
pub struct Corpus {
    raw: *mut sys::PqvCorpus,
}
unsafe impl Send for Corpus {}
unsafe impl Sync for Corpus {}

impl Corpus {
    /// `Embeddings::new(data, dim)` + upload: `rows` is row-major `[n, dim]`.
    pub fn upload(device: usize, rows: &[f32], dim: usize) -> Result<Self> {
        if dim == 0 {
            return Err("Embedding dimension must be > 0".into()); // src/ivf/mod.rs:59
        }
        if rows.len() % dim != 0 {
            return Err("Embedding data length must be a multiple of dimension".into()); // src/ivf/mod.rs:86
        }
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::pqv_corpus_upload(device as c_int, rows.as_ptr(), (rows.len() / dim) as u64, dim as u32, &mut raw)
        })?;
        Ok(Self { raw })
    }

    /// Streaming form for `read_parquet_with_embeddings` (`src/ivf/parquet.rs:216-305`): reserve, then append
    /// one row group's values buffer at a time -- no `Vec<f32>` of the whole column.
    pub fn with_capacity(device: usize, capacity_rows: usize, dim: usize) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_corpus_create(device as c_int, capacity_rows as u64, dim as u32, &mut raw) })?;
        Ok(Self { raw })
    }

    pub fn append(&mut self, rows: &[f32]) -> Result<()> {
        let dim = self.dim();
        if rows.len() % dim != 0 {
            return Err("Embedding data length must be a multiple of dimension".into());
        }
        check(unsafe { sys::pqv_corpus_append(self.raw, rows.as_ptr(), (rows.len() / dim) as u64) })
    }

    /// Float64 columns are narrowed with `as f32` (`src/ivf/parquet.rs:246-256`).
    pub fn append_f64(&mut self, rows: &[f64]) -> Result<()> {
        let dim = self.dim();
        if rows.len() % dim != 0 {
            return Err("Embedding data length must be a multiple of dimension".into());
        }
        check(unsafe { sys::pqv_corpus_append_f64(self.raw, rows.as_ptr(), (rows.len() / dim) as u64) })
    }

    /// Streaming upload (`src/ivf/parquet.rs:262-286` batch by batch): rows `[row_offset, row_offset + rows.len() / dim)` are
    /// staged in pinned memory and DMA'd asynchronously; batches may come in any order, from several threads (`&self`).
    pub fn write_rows(&self, row_offset: usize, rows: &[f32]) -> Result<()> {
        let dim = self.dim();
        if rows.len() % dim != 0 {
            return Err("Embedding data length must be a multiple of dimension".into());
        }
        check(unsafe { sys::pqv_corpus_write_rows(self.raw, row_offset as u64, rows.as_ptr(), (rows.len() / dim) as u64) })
    }

    pub fn write_rows_f64(&self, row_offset: usize, rows: &[f64]) -> Result<()> {
        let dim = self.dim();
        if rows.len() % dim != 0 {
            return Err("Embedding data length must be a multiple of dimension".into());
        }
        check(unsafe { sys::pqv_corpus_write_rows_f64(self.raw, row_offset as u64, rows.as_ptr(), (rows.len() / dim) as u64) })
    }

    /// A run of uncompressed PLAIN v1 data pages of the embedding leaf, straight from the memory-mapped file `file`: page `i`'s
    /// body is `file[body_off[i] .. body_off[i] + body_len[i]]`.  Per page the level runs are verified -- a row starts exactly
    /// every `dim` values, every definition level is `max_def`: the checks of `src/ivf/parquet.rs:231-280`, made on the levels --
    /// and the values behind them go to rows `first_value[i] / dim ..`.  `Ok(None)`: all uploaded; `Ok(Some(i))`: page `i` is not
    /// such a page and nothing of the run was uploaded (read the column through the Arrow reader, which owns the error texts).
    pub fn write_plain_pages(&self, file: &[u8], body_off: &[u64], body_len: &[u32], first_value: &[u64], n_values: &[u32],
                             max_def: u32, f64_values: bool) -> Result<Option<usize>> {
        let n = body_off.len();
        if body_len.len() != n || first_value.len() != n || n_values.len() != n {
            return Err("page tables must have one entry per page".into());
        }
        for i in 0..n {
            if body_off[i].checked_add(body_len[i] as u64).map_or(true, |e| e > file.len() as u64) {
                return Err("a page body lies outside the mapped file".into());
            }
        }
        let mut bad = 0u32;
        let rc = unsafe {
            sys::pqv_corpus_write_plain_pages(self.raw, file.as_ptr(), body_off.as_ptr(), body_len.as_ptr(), first_value.as_ptr(),
                                              n_values.as_ptr(), n as u32, self.dim() as u32, max_def, f64_values as c_int, &mut bad)
        };
        if rc == 1 {
            return Ok(Some(bad as usize));
        }
        check(rc).map(|_| None)
    }

    /// Waits for every upload and sets the row count.
    pub fn finish(&mut self, n_rows: usize) -> Result<()> {
        check(unsafe { sys::pqv_corpus_finish(self.raw, n_rows as u64) })
    }

    /// (crate-internal: the handle, for entry points that take `pqv_corpus *`)
    #[allow(dead_code)]
    pub(crate) fn raw_mut(&mut self) -> *mut sys::PqvCorpus {
        self.raw
    }

    pub fn rows(&self) -> usize {
        unsafe { sys::pqv_corpus_rows(self.raw) as usize }
    }
    pub fn dim(&self) -> usize {
        unsafe { sys::pqv_corpus_dim(self.raw) as usize }
    }
}

impl Drop for Corpus {
    fn drop(&mut self) {
        unsafe { sys::pqv_corpus_free(self.raw) }
    }
}

/// `IvfIndex` (`src/ivf/index.rs:9-14`): dim, n_clusters, centroids, inverted lists.
pub struct Index {
    raw: *mut sys::PqvIndex,
}
unsafe impl Send for Index {}
unsafe impl Sync for Index {}

impl Index {
    /// `IvfIndex::from_bytes` (`src/ivf/index.rs:85-128`).
    pub fn from_bytes(bytes: &[u8]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_index_from_bytes(bytes.as_ptr(), bytes.len(), &mut raw) })?;
        Ok(Self { raw })
    }

    /// `IvfIndex::to_bytes` (`src/ivf/index.rs:65-83`); byte-identical layout, so the existing
    /// `append_index_inplace` / `write_parquet_with_index` embed it unchanged.
    pub fn to_bytes(&self) -> Result<Vec<u8>> {
        let (mut buf, mut len) = (ptr::null_mut(), 0usize);
        check(unsafe { sys::pqv_index_to_bytes(self.raw, &mut buf, &mut len) })?;
        let out = if buf.is_null() || len == 0 { Vec::new() } else { unsafe { std::slice::from_raw_parts(buf, len) }.to_vec() };
        unsafe { sys::pqv_bytes_free(buf) };
        Ok(out)
    }

    pub fn dim(&self) -> usize {
        unsafe { sys::pqv_index_dim(self.raw) as usize }
    }
    pub fn n_clusters(&self) -> usize {
        unsafe { sys::pqv_index_n_clusters(self.raw) as usize }
    }
    pub fn centroids(&self) -> &[f32] {
        let n = self.dim() * self.n_clusters();
        unsafe { std::slice::from_raw_parts(sys::pqv_index_centroids(self.raw), n) }
    }
    /// `inverted_lists[c]`, ascending row ids.
    pub fn inverted_list(&self, cluster: usize) -> &[u32] {
        let off = unsafe { std::slice::from_raw_parts(sys::pqv_index_list_offsets(self.raw), self.n_clusters() + 1) };
        let rows = unsafe { std::slice::from_raw_parts(sys::pqv_index_list_rows(self.raw), sys::pqv_index_n_rows(self.raw) as usize) };
        &rows[off[cluster] as usize..off[cluster + 1] as usize]
    }

    /// `nearest_centroid` (`src/ivf/index.rs:244-257`) of corpus rows `[first_row, first_row + n_rows)` under this index'
    /// centroids: the lowest index wins a tie, a row no centroid is below +inf from goes to 0.
    pub fn assign(&self, corpus: &Corpus, first_row: usize, n_rows: usize) -> Result<Vec<u32>> {
        let mut out = vec![0u32; n_rows];
        check(unsafe { sys::pqv_index_assign(self.raw, corpus.raw, first_row as u64, n_rows as u64, out.as_mut_ptr()) })?;
        Ok(out)
    }

    /// A new index with these centroids whose list `c` is this index' list `c` followed by the rows of
    /// `[first_row, first_row + n_rows)` assigned to `c`, ascending (`src/ivf/index.rs:189-206` for these centroids over the longer
    /// column; no k-means).  `first_row` must be at least the largest indexed row id + 1.  `self` is not modified; a searcher over
    /// the grown corpus is made from the result.
    pub fn append(&self, corpus: &Corpus, first_row: usize, n_rows: usize) -> Result<Index> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_index_append(self.raw, corpus.raw, first_row as u64, n_rows as u64, &mut raw) })?;
        Ok(Index { raw })
    }

    /// A new index with these centroids whose lists no longer hold the rows `r < remove.len()` with `remove[r] != 0`; order is
    /// kept, row ids stay what they were and the row bound is carried over.  Runs on `device` where there is one, else on the
    /// host with the same result.  `self` is not modified: searchers made from it keep answering as before.
    pub fn remove(&self, device: usize, remove: &[u8]) -> Result<Index> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_index_remove(self.raw, device as c_int, remove.as_ptr(), remove.len() as u64, &mut raw) })?;
        Ok(Index { raw })
    }

    /// `remove` by row id: any order, duplicates allowed, ids that are not indexed ignored.
    pub fn remove_rows(&self, device: usize, rows: &[u32]) -> Result<Index> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_index_remove_rows(self.raw, device as c_int, rows.as_ptr(), rows.len() as u64, &mut raw) })?;
        Ok(Index { raw })
    }

    /// The vacuum: a dense corpus of the rows this index still holds (ascending old id, bit for bit, room for
    /// `max(capacity_rows, kept)` rows), the index renumbered onto it (new id = rank of the old id among the kept rows), and
    /// `old_row[j]` = the old id of new row `j` -- attached columns are re-made as `column[old_row]`.
    pub fn compact(&self, corpus: &Corpus, capacity_rows: usize) -> Result<(Corpus, Index, Vec<u32>)> {
        let (mut c_raw, mut i_raw) = (ptr::null_mut(), ptr::null_mut());
        let mut old_row = vec![0u32; unsafe { sys::pqv_index_n_rows(self.raw) } as usize];
        check(unsafe {
            sys::pqv_index_compact(self.raw, corpus.raw, capacity_rows as u64, &mut c_raw, &mut i_raw, old_row.as_mut_ptr())
        })?;
        let (c, i) = (Corpus { raw: c_raw }, Index { raw: i_raw });
        old_row.truncate(c.rows());
        Ok((c, i, old_row))
    }
}

impl Drop for Index {
    fn drop(&mut self) {
        unsafe { sys::pqv_index_free(self.raw) }
    }
}

/// `IndexBuilder` (`src/ivf/parquet.rs:23-103`) over a resident column: same knobs, same defaults
/// (`max_iters` 20, `seed` 42, `n_clusters` = ceil(sqrt(n)) when unset), same validation texts.
#[derive(Debug, Clone)]
pub struct IndexBuilder {
    n_clusters: Option<usize>,
    max_iters: usize,
    seed: u64,
    workers: usize,
}

impl Default for IndexBuilder {
    fn default() -> Self {
        Self::new()
    }
}

impl IndexBuilder {
    pub fn new() -> Self {
        // `workers` is what the reference's worker_count() would see (src/ivf/index.rs:259-265): it fixes the
        // chunking of one f32 sum in k-means++, so it is part of the reproducible configuration.
        let workers = std::thread::available_parallelism().map(|n| n.get()).unwrap_or(1);
        Self { n_clusters: None, max_iters: 20, seed: 42, workers }
    }
    pub fn n_clusters(mut self, n_clusters: usize) -> Self {
        self.n_clusters = Some(n_clusters);
        self
    }
    pub fn max_iters(mut self, max_iters: usize) -> Self {
        self.max_iters = max_iters;
        self
    }
    pub fn seed(mut self, seed: u64) -> Self {
        self.seed = seed;
        self
    }
    pub fn workers(mut self, workers: usize) -> Self {
        self.workers = workers;
        self
    }

    /// `build_config()` + `build_ivf_index()`; the caller embeds `index.to_bytes()` exactly as
    /// `build_inplace` / `build_new` do today.
    pub fn build(self, corpus: &Corpus) -> Result<Index> {
        if self.max_iters == 0 {
            return Err("max_iters must be > 0".into()); // parquet.rs:90
        }
        let n_clusters = match self.n_clusters {
            Some(0) => return Err("n_clusters must be > 0".into()), // parquet.rs:93
            Some(v) => u32::try_from(v)?,
            None => 0, // the library applies ceil(sqrt(n)) (index.rs:161-167)
        };
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::pqv_index_build(corpus.raw, n_clusters, u32::try_from(self.max_iters)?, self.seed, self.workers as u32, &mut raw)
        })?;
        Ok(Index { raw })
    }
}

/// `SearchResult` (`src/ivf/search.rs:41-45`).
#[derive(Debug, Clone, PartialEq)]
pub struct SearchResult {
    pub row_idx: u32,
    pub distance: f32,
}

/// One group of a distinct top-k ([`Searcher::topk_distinct`]): the group's nearest row, its distance and the group's key value.
#[derive(Debug, Clone, PartialEq)]
pub struct DistinctSearchResult {
    pub row_idx: u32,
    pub distance: f32,
    pub key: i64,
}

/// One group of a grouped top-k ([`Searcher::topk_grouped`]): the group's key value and its nearest rows, nearest first.
#[derive(Debug, Clone, PartialEq)]
pub struct GroupSearchResult {
    pub key: i64,
    pub hits: Vec<SearchResult>,
}

/// An index bound to its column on one GPU.  What `topk()` re-creates per query from the file
/// (`read_index_from_parquet` + `read_embeddings_for_rows`, `src/ivf/search.rs:89-110`) is kept resident here:
/// cache one per indexed Parquet file.
pub struct Searcher<'c> {
    raw: *mut sys::PqvSearcher,
    _corpus: std::marker::PhantomData<&'c Corpus>,
}
unsafe impl Send for Searcher<'_> {}
unsafe impl Sync for Searcher<'_> {}

impl<'c> Searcher<'c> {
    pub fn new(index: &Index, corpus: &'c mut Corpus) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_searcher_create(index.raw, corpus.raw, sys::PQV_LAYOUT_IVF_ORDERED, &mut raw) })?;
        Ok(Self { raw, _corpus: std::marker::PhantomData })
    }

    /// `IvfIndex::candidate_rows` (`src/ivf/index.rs:57-63`): probe-rank major, ascending ids inside.
    pub fn candidate_rows(&self, query: &[f32], nprobe: NonZeroUsize) -> Result<Vec<u32>> {
        let (mut rows, mut n) = (ptr::null_mut(), 0u64);
        check(unsafe {
            sys::pqv_candidate_rows(self.raw, query.as_ptr(), query.len() as u32, nprobe.get() as u32, &mut rows, &mut n)
        })?;
        let out = if rows.is_null() || n == 0 { Vec::new() } else { unsafe { std::slice::from_raw_parts(rows, n as usize) }.to_vec() };
        unsafe { sys::pqv_rows_free(rows) };
        Ok(out)
    }

    /// `topk()` (`src/ivf/search.rs:83-142`) for a batch of queries (`queries.len() == nq * dim`): identical
    /// results to the reference, ties included (flagged queries are replayed through the reference's heap).
    pub fn topk(&self, queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        self.topk_metric(queries, dim, k, nprobe, sys::PQV_L2SQ_REF4)
    }

    /// [`Searcher::topk`] by cosine distance (an extension; `include/pqv.h`: `PQV_COSINE`): the distance is `0.5 * d2` of the
    /// normalised query and row, `1 - cos` in exact arithmetic.  The first such call builds the searcher's cosine layout.
    pub fn topk_cosine(&self, queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        self.topk_metric(queries, dim, k, nprobe, sys::PQV_COSINE)
    }

    /// [`Searcher::topk`] by inner product (an extension; `include/pqv.h`: `PQV_DOT`): the distance is `-(q.x)`, the negated
    /// similarity in the 4-grouped f32 chain, smallest first; ties by candidate position, no heap replay.  `k <= 1024` and at most
    /// 1024 probed lists per query.
    pub fn topk_dot(&self, queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        self.topk_metric(queries, dim, k, nprobe, sys::PQV_DOT)
    }

    fn topk_metric(&self, queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize, metric: c_int)
        -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (k, np) = (k.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk(self.raw, queries.as_ptr(), nq as u32, dim as u32, k as u32, np as u32, 0, metric, 1,
                          rows.as_mut_ptr(), dist.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// Range search (no counterpart in the reference): for every query (`queries.len() == nq * dim`) each candidate
    /// of `nprobe` lists whose distance (sqrt of the `PQV_L2SQ_REF4` d2, as [`Searcher::topk`]) is `<= radius`, ascending
    /// by (distance, candidate position); `max_results > 0` keeps the first that many per query.  A NaN radius is an error.
    pub fn range_search(&self, queries: &[f32], dim: usize, radius: f32, nprobe: NonZeroUsize, max_results: u64)
        -> Result<Vec<Vec<SearchResult>>> {
        self.range_search_metric(queries, dim, radius, nprobe, max_results, sys::PQV_L2SQ_REF4)
    }

    /// [`Searcher::range_search`] by cosine distance (`include/pqv.h`: `PQV_COSINE`): hits are the candidates with
    /// `0.5 * d2 <= radius` (d2 of the normalised vectors), and that is the distance returned.
    pub fn range_search_cosine(&self, queries: &[f32], dim: usize, radius: f32, nprobe: NonZeroUsize, max_results: u64)
        -> Result<Vec<Vec<SearchResult>>> {
        self.range_search_metric(queries, dim, radius, nprobe, max_results, sys::PQV_COSINE)
    }

    /// [`Searcher::range_search`] by inner product (`include/pqv.h`: `PQV_DOT`): hits are the candidates with `-(q.x) <= radius`
    /// (`radius = -0.8` keeps `q.x >= 0.8`), and that is the distance returned.
    pub fn range_search_dot(&self, queries: &[f32], dim: usize, radius: f32, nprobe: NonZeroUsize, max_results: u64)
        -> Result<Vec<Vec<SearchResult>>> {
        self.range_search_metric(queries, dim, radius, nprobe, max_results, sys::PQV_DOT)
    }

    fn range_search_metric(&self, queries: &[f32], dim: usize, radius: f32, nprobe: NonZeroUsize, max_results: u64, metric: c_int)
        -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (mut lims, mut rows, mut dist) = (ptr::null_mut::<u64>(), ptr::null_mut::<u32>(), ptr::null_mut::<f32>());
        check(unsafe {
            sys::pqv_range_search(self.raw, queries.as_ptr(), nq as u32, dim as u32, radius, nprobe.get() as u32, 0, max_results,
                                  metric, 1, &mut lims, &mut rows, &mut dist, ptr::null_mut(), ptr::null_mut())
        })?;
        if lims.is_null() || rows.is_null() || dist.is_null() {
            unsafe { sys::pqv_range_free(lims, rows, dist) };
            return Err("pqv_range_search returned a NULL buffer".into());
        }
        let out = {
            let l = unsafe { std::slice::from_raw_parts(lims, nq + 1) };
            let total = l[nq] as usize;
            let (r, d) = if total == 0 {
                (&[][..], &[][..])
            } else {
                unsafe { (std::slice::from_raw_parts(rows, total), std::slice::from_raw_parts(dist, total)) }
            };
            (0..nq)
                .map(|q| (l[q] as usize..l[q + 1] as usize).map(|i| SearchResult { row_idx: r[i], distance: d[i] }).collect())
                .collect()
        };
        unsafe { sys::pqv_range_free(lims, rows, dist) };
        Ok(out)
    }

    /// A row mask for this searcher (`include/pqv.h`: `pqv_row_mask`): `allowed[r]` says whether the row reported as `row_idx == r`
    /// may be returned; `allowed.len()` must be the corpus' row count.  What a DataFusion host gets from its `FilterExec`.
    pub fn row_mask(&self, allowed: &[bool]) -> Result<RowMask> {
        let bytes: Vec<u8> = allowed.iter().map(|&b| b as u8).collect();
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_row_mask_create(self.raw, bytes.as_ptr(), bytes.len() as u64, &mut raw) })?;
        Ok(RowMask { raw })
    }

    /// [`Searcher::topk`] over the allowed rows only (the reference's predicate inside the scan, `src/df_vector/exec.rs:207-277`):
    /// fewer than `k` results may come back.
    pub fn topk_masked(&self, mask: &RowMask, queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize)
        -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (k, np) = (k.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_masked(self.raw, mask.raw, queries.as_ptr(), nq as u32, dim as u32, k as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1,
                                 rows.as_mut_ptr(), dist.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// [`Searcher::range_search`] over the allowed rows only.
    pub fn range_search_masked(&self, mask: &RowMask, queries: &[f32], dim: usize, radius: f32, nprobe: NonZeroUsize, max_results: u64)
        -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (mut lims, mut rows, mut dist) = (ptr::null_mut::<u64>(), ptr::null_mut::<u32>(), ptr::null_mut::<f32>());
        check(unsafe {
            sys::pqv_range_search_masked(self.raw, mask.raw, queries.as_ptr(), nq as u32, dim as u32, radius, nprobe.get() as u32, 0,
                                         max_results, sys::PQV_L2SQ_REF4, 1, &mut lims, &mut rows, &mut dist, ptr::null_mut(), ptr::null_mut())
        })?;
        if lims.is_null() || rows.is_null() || dist.is_null() {
            unsafe { sys::pqv_range_free(lims, rows, dist) };
            return Err("pqv_range_search_masked returned a NULL buffer".into());
        }
        let out = {
            let l = unsafe { std::slice::from_raw_parts(lims, nq + 1) };
            let total = l[nq] as usize;
            let (r, d) = if total == 0 {
                (&[][..], &[][..])
            } else {
                unsafe { (std::slice::from_raw_parts(rows, total), std::slice::from_raw_parts(dist, total)) }
            };
            (0..nq)
                .map(|q| (l[q] as usize..l[q + 1] as usize).map(|i| SearchResult { row_idx: r[i], distance: d[i] }).collect())
                .collect()
        };
        unsafe { sys::pqv_range_free(lims, rows, dist) };
        Ok(out)
    }

    /// The keys of an integer column laid out for this searcher (`include/pqv.h`: `pqv_row_keys`); the column is copied.
    pub fn row_keys(&self, column: &Column) -> Result<RowKeys> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_row_keys_create(self.raw, column.raw, ptr::null_mut(), &mut raw) })?;
        Ok(RowKeys { raw })
    }

    /// [`Searcher::topk_masked`] with one filter PER QUERY: query `q` considers the rows whose key equals `query_keys[q]` -- and
    /// that `mask` allows, where one is given (`include/pqv.h`: `pqv_topk_keyed`).
    pub fn topk_keyed(&self, keys: &RowKeys, query_keys: &[i64], mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize,
                      nprobe: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        if query_keys.len() != nq {
            return Err("one query key per query".into());
        }
        let (k, np) = (k.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_keyed(self.raw, keys.raw, query_keys.as_ptr(), mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                                nq as u32, dim as u32, k as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(),
                                dist.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// [`Searcher::topk_keyed`] under any per-query filter: a key, an inclusive range or a set per query (`include/pqv.h`:
    /// `pqv_topk_filtered`).  Sets are sorted and de-duplicated here; one beyond `PQV_KEY_SET_MAX` values is refused.
    pub fn topk_filtered(&self, keys: &RowKeys, filter: &KeyFilter, mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize,
                         nprobe: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let (desc, _lims, _vals) = key_filter_desc(filter, nq)?;
        let (k, np) = (k.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_filtered(self.raw, keys.raw, &desc, mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                                   nq as u32, dim as u32, k as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(),
                                   dist.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// A posting list per key value of an integer column over this searcher's rows (`include/pqv.h`: `pqv_key_partition`).
    pub fn key_partition(&self, column: &Column) -> Result<KeyPartition> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_key_partition_create(self.raw, column.raw, ptr::null_mut(), &mut raw) })?;
        Ok(KeyPartition { raw })
    }

    /// The exact top-k over the rows of `part` whose key passes the query's filter -- nothing is probed (`include/pqv.h`:
    /// `pqv_topk_partition`).  Sets are sorted and de-duplicated here, as for [`Searcher::topk_filtered`].
    pub fn topk_partition(&self, part: &KeyPartition, filter: &KeyFilter, mask: Option<&RowMask>, queries: &[f32], dim: usize,
                          k: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let (desc, _lims, _vals) = key_filter_desc(filter, nq)?;
        let k = k.get();
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_partition(self.raw, part.raw, &desc, mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                                    nq as u32, dim as u32, k as u32, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(), dist.as_mut_ptr(),
                                    found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// The exact top-k among the rows the caller names per query -- `candidates[q]` in any order, duplicates allowed, rows that are
    /// not indexed skipped -- within `mask` if one is given; nothing is probed (`include/pqv.h`: `pqv_topk_rows`).
    pub fn topk_rows(&self, candidates: &[Vec<u32>], mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize)
                     -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (lims, cand) = candidate_lists(candidates, nq)?;
        let k = k.get();
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_rows(self.raw, lims.as_ptr(), cand.as_ptr(), mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                               nq as u32, dim as u32, k as u32, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(), dist.as_mut_ptr(),
                               found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// The exact distance of every candidate to its query, in the order given; `+inf` for a row that is not indexed or that `mask`
    /// excludes (`include/pqv.h`: `pqv_score_rows`).
    pub fn score_rows(&self, candidates: &[Vec<u32>], mask: Option<&RowMask>, queries: &[f32], dim: usize) -> Result<Vec<Vec<f32>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (lims, cand) = candidate_lists(candidates, nq)?;
        let mut dist = vec![f32::INFINITY; cand.len().max(1)];
        check(unsafe {
            sys::pqv_score_rows(self.raw, lims.as_ptr(), cand.as_ptr(), mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                                nq as u32, dim as u32, sys::PQV_L2SQ_REF4, 1, dist.as_mut_ptr())
        })?;
        Ok((0..nq).map(|q| dist[lims[q] as usize..lims[q + 1] as usize].to_vec()).collect())
    }

    /// MMR top-k: the `fetch_k` nearest rows of the probed lists (within `mask` if one is given), then `k` of them picked greedily by
    /// `lambda * distance - (1 - lambda) * distance to the nearest pick so far`, smallest first; the results come in pick order
    /// (`include/pqv.h`: `pqv_topk_mmr`).
    pub fn topk_mmr(&self, mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize, fetch_k: NonZeroUsize, lambda: f32,
                    nprobe: NonZeroUsize) -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let k = k.get();
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_mmr(self.raw, mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(), nq as u32, dim as u32, k as u32,
                              fetch_k.get() as u32, lambda, nprobe.get() as u32, 0, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(),
                              dist.as_mut_ptr(), ptr::null_mut(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// The MMR selection alone over `candidates[q]`, the results of any top-k call of this searcher (all of one length), in pick
    /// order (`include/pqv.h`: `pqv_mmr_select`).
    pub fn mmr_select(&self, candidates: &[Vec<SearchResult>], k: NonZeroUsize, lambda: f32) -> Result<Vec<Vec<SearchResult>>> {
        let nq = candidates.len();
        let n = candidates.first().map_or(0, |c| c.len());
        if candidates.iter().any(|c| c.len() != n) {
            return Err("mmr_select needs candidate lists of one length".into());
        }
        let k = k.get();
        let cand: Vec<u32> = candidates.iter().flat_map(|c| c.iter().map(|r| r.row_idx)).collect();
        let rel: Vec<f32> = candidates.iter().flat_map(|c| c.iter().map(|r| r.distance)).collect();
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_mmr_select(self.raw, cand.as_ptr(), rel.as_ptr(), ptr::null(), nq as u32, n as u32, k as u32, lambda,
                                sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(), dist.as_mut_ptr(), ptr::null_mut(), found.as_mut_ptr())
        })?;
        Ok((0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect())
    }

    /// Every row of `part` whose key passes the query's filter within `radius` of the query -- exact, nothing is probed, ascending by
    /// (distance, sequence position); `max_results > 0` keeps the first `max_results` of each query (`include/pqv.h`:
    /// `pqv_range_search_partition`).
    pub fn range_search_partition(&self, part: &KeyPartition, filter: &KeyFilter, mask: Option<&RowMask>, queries: &[f32], dim: usize,
                                  radius: f32, max_results: u64) -> Result<Vec<Vec<SearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let (desc, _lims, _vals) = key_filter_desc(filter, nq)?;
        let (mut lims, mut rows, mut dist) = (ptr::null_mut::<u64>(), ptr::null_mut::<u32>(), ptr::null_mut::<f32>());
        check(unsafe {
            sys::pqv_range_search_partition(self.raw, part.raw, &desc, mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                                            nq as u32, dim as u32, radius, max_results, sys::PQV_L2SQ_REF4, 1, &mut lims, &mut rows,
                                            &mut dist, ptr::null_mut(), ptr::null_mut())
        })?;
        if lims.is_null() || rows.is_null() || dist.is_null() {
            unsafe { sys::pqv_range_free(lims, rows, dist) };
            return Err("pqv_range_search_partition returned a NULL buffer".into());
        }
        let out = {
            let l = unsafe { std::slice::from_raw_parts(lims, nq + 1) };
            let total = l[nq] as usize;
            let (r, d) = if total == 0 {
                (&[][..], &[][..])
            } else {
                unsafe { (std::slice::from_raw_parts(rows, total), std::slice::from_raw_parts(dist, total)) }
            };
            (0..nq)
                .map(|q| (l[q] as usize..l[q + 1] as usize).map(|i| SearchResult { row_idx: r[i], distance: d[i] }).collect())
                .collect()
        };
        unsafe { sys::pqv_range_free(lims, rows, dist) };
        Ok(out)
    }

    /// Up to `group_size` rows of each of the `k` nearest groups of `group_keys` among the rows of `part` whose key passes the
    /// query's filter -- exact, nothing is probed; `group_size` 1 is the distinct call (`include/pqv.h`:
    /// `pqv_topk_partition_grouped`).  `k * group_size <= 1024`.
    pub fn topk_partition_grouped(&self, part: &KeyPartition, filter: &KeyFilter, group_keys: &RowKeys, mask: Option<&RowMask>,
                                  queries: &[f32], dim: usize, k: NonZeroUsize, group_size: NonZeroUsize)
                                  -> Result<Vec<Vec<GroupSearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let (desc, _lims, _vals) = key_filter_desc(filter, nq)?;
        let (k, m) = (k.get(), group_size.get());
        let mut rows = vec![0u32; nq * k * m];
        let mut dist = vec![0f32; nq * k * m];
        let mut group = vec![0i64; nq * k];
        let mut group_rows = vec![0u32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_partition_grouped(self.raw, part.raw, &desc, group_keys.raw, mask.map_or(ptr::null(), |x| x.raw as *const _),
                                            queries.as_ptr(), nq as u32, dim as u32, k as u32, m as u32, sys::PQV_L2SQ_REF4, 1,
                                            rows.as_mut_ptr(), dist.as_mut_ptr(), group.as_mut_ptr(), group_rows.as_mut_ptr(),
                                            found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|g| {
                        let o = (q * k + g) * m;
                        GroupSearchResult {
                            key: group[q * k + g],
                            hits: (0..group_rows[q * k + g] as usize)
                                .map(|i| SearchResult { row_idx: rows[o + i], distance: dist[o + i] })
                                .collect(),
                        }
                    })
                    .collect()
            })
            .collect())
    }

    /// Keep probing until `k` rows pass the filter (`include/pqv.h`: `pqv_topk_expand`): every query probes the fewest lists, at
    /// least `nprobe` and at most `max_nprobe`, whose passing rows number `k`, and gets what [`Searcher::topk_masked`] (`filter`
    /// `None`: `mask` is required) or [`Searcher::topk_filtered`] returns for that many lists.  Returns the hits and the lists
    /// each query probed.
    pub fn topk_expand(&self, filter: Option<(&RowKeys, &KeyFilter)>, mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize,
                       nprobe: NonZeroUsize, max_nprobe: NonZeroUsize) -> Result<(Vec<Vec<SearchResult>>, Vec<u32>)> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let held = match filter {
            Some((_, f)) => Some(key_filter_desc(f, nq)?),
            None => None,
        };
        let keys_raw = filter.map_or(ptr::null(), |(kk, _)| kk.raw as *const _);
        let desc_ptr = held.as_ref().map_or(ptr::null(), |h| &h.0 as *const sys::PqvKeyFilter);
        let (k, np, max_np) = (k.get(), nprobe.get(), max_nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        let mut used = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_expand(self.raw, keys_raw, desc_ptr, mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(),
                                 nq as u32, dim as u32, k as u32, np as u32, max_np as u32, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(),
                                 dist.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut(), used.as_mut_ptr())
        })?;
        let hits = (0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect();
        Ok((hits, used))
    }

    /// The plain top-k call with a probe depth per query (`include/pqv.h`: `pqv_topk_depth`): query `q` walks
    /// `min(max(r, nprobe), max_nprobe)` lists -- `r` its entry of [`ProbeDepth::Given`], or with [`ProbeDepth::Ratio`] the lists whose
    /// centroid lies within that factor (squared scale, `>= 1`) of the nearest centroid's distance -- and gets what
    /// [`Searcher::topk`] returns at that `nprobe`.  Returns the hits and the lists each query probed.
    pub fn topk_depth(&self, depth: &ProbeDepth, queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize,
                      max_nprobe: NonZeroUsize) -> Result<(Vec<Vec<SearchResult>>, Vec<u32>)> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (k, np, max_np) = (k.get(), nprobe.get(), max_nprobe.get());
        // (the array the descriptor points at lives until the call has returned)
        let desc = match depth {
            ProbeDepth::Given(d) => {
                if d.len() != nq {
                    return Err("one probe depth per query".into());
                }
                sys::PqvProbeDepth { kind: sys::PQV_DEPTH_GIVEN, max_nprobe: max_np as u32, d2_ratio: 0.0, depths: d.as_ptr() as *const c_void }
            }
            ProbeDepth::Ratio(r) => sys::PqvProbeDepth { kind: sys::PQV_DEPTH_RATIO, max_nprobe: max_np as u32, d2_ratio: *r, depths: ptr::null() },
        };
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut found = vec![0u32; nq];
        let mut used = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_depth(self.raw, &desc as *const sys::PqvProbeDepth, queries.as_ptr(), nq as u32, dim as u32, k as u32, np as u32,
                                sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(), dist.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut(),
                                used.as_mut_ptr())
        })?;
        let hits = (0..nq)
            .map(|q| (0..found[q] as usize).map(|i| SearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i] }).collect())
            .collect();
        Ok((hits, used))
    }

    /// The nearest row of each of the `k` nearest groups -- a group is the considered rows of one value of `keys` (NULL-key rows
    /// belong to none), under `mask` where one is given (`include/pqv.h`: `pqv_topk_distinct`).  Ascending by (distance, position).
    pub fn topk_distinct(&self, keys: &RowKeys, mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize,
                         nprobe: NonZeroUsize) -> Result<Vec<Vec<DistinctSearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (k, np) = (k.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut group = vec![0i64; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_distinct(self.raw, keys.raw, mask.map_or(ptr::null(), |m| m.raw as *const _), queries.as_ptr(), nq as u32,
                                   dim as u32, k as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(), dist.as_mut_ptr(),
                                   group.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|i| DistinctSearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i], key: group[q * k + i] })
                    .collect()
            })
            .collect())
    }

    /// [`Searcher::topk_distinct`] with one filter PER QUERY on `filter_keys` (which may be `group_keys`), applied before a group's
    /// representative is chosen: the nearest documents of every query's own tenant (`include/pqv.h`: `pqv_topk_distinct_filtered`).
    pub fn topk_distinct_filtered(&self, group_keys: &RowKeys, filter_keys: &RowKeys, filter: &KeyFilter, mask: Option<&RowMask>,
                                  queries: &[f32], dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize) -> Result<Vec<Vec<DistinctSearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let (desc, _lims, _vals) = key_filter_desc(filter, nq)?;
        let (k, np) = (k.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut group = vec![0i64; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_distinct_filtered(self.raw, group_keys.raw, filter_keys.raw, &desc, mask.map_or(ptr::null(), |m| m.raw as *const _),
                                            queries.as_ptr(), nq as u32, dim as u32, k as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1,
                                            rows.as_mut_ptr(), dist.as_mut_ptr(), group.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|i| DistinctSearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i], key: group[q * k + i] })
                    .collect()
            })
            .collect())
    }

    /// Keep probing until `k` GROUPS are found (`include/pqv.h`: `pqv_topk_distinct_expand`): every query probes the fewest lists, at
    /// least `nprobe` and at most `max_nprobe`, that hold `k` distinct values of `group_keys` among the rows it considers, and gets
    /// what [`Searcher::topk_distinct`] (`filter` `None`) or [`Searcher::topk_distinct_filtered`] returns for that many lists.
    /// Returns the hits and the lists each query probed.
    pub fn topk_distinct_expand(&self, group_keys: &RowKeys, filter: Option<(&RowKeys, &KeyFilter)>, mask: Option<&RowMask>, queries: &[f32],
                                dim: usize, k: NonZeroUsize, nprobe: NonZeroUsize, max_nprobe: NonZeroUsize)
                                -> Result<(Vec<Vec<DistinctSearchResult>>, Vec<u32>)> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        // (the arrays the descriptor points at live until the call has returned)
        let held = match filter {
            Some((_, f)) => Some(key_filter_desc(f, nq)?),
            None => None,
        };
        let keys_raw = filter.map_or(ptr::null(), |(kk, _)| kk.raw as *const _);
        let desc_ptr = held.as_ref().map_or(ptr::null(), |h| &h.0 as *const sys::PqvKeyFilter);
        let (k, np, max_np) = (k.get(), nprobe.get(), max_nprobe.get());
        let mut rows = vec![0u32; nq * k];
        let mut dist = vec![0f32; nq * k];
        let mut group = vec![0i64; nq * k];
        let mut found = vec![0u32; nq];
        let mut used = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_distinct_expand(self.raw, group_keys.raw, keys_raw, desc_ptr, mask.map_or(ptr::null(), |m| m.raw as *const _),
                                          queries.as_ptr(), nq as u32, dim as u32, k as u32, np as u32, max_np as u32, sys::PQV_L2SQ_REF4, 1,
                                          rows.as_mut_ptr(), dist.as_mut_ptr(), group.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut(),
                                          used.as_mut_ptr())
        })?;
        let hits = (0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|i| DistinctSearchResult { row_idx: rows[q * k + i], distance: dist[q * k + i], key: group[q * k + i] })
                    .collect()
            })
            .collect();
        Ok((hits, used))
    }

    /// [`Searcher::topk_distinct_expand`] with up to `group_size` rows per group (`include/pqv.h`: `pqv_topk_grouped_expand`): the
    /// target stays `k` groups.
    pub fn topk_grouped_expand(&self, group_keys: &RowKeys, filter: Option<(&RowKeys, &KeyFilter)>, mask: Option<&RowMask>, queries: &[f32],
                               dim: usize, k: NonZeroUsize, group_size: NonZeroUsize, nprobe: NonZeroUsize, max_nprobe: NonZeroUsize)
                               -> Result<(Vec<Vec<GroupSearchResult>>, Vec<u32>)> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let held = match filter {
            Some((_, f)) => Some(key_filter_desc(f, nq)?),
            None => None,
        };
        let keys_raw = filter.map_or(ptr::null(), |(kk, _)| kk.raw as *const _);
        let desc_ptr = held.as_ref().map_or(ptr::null(), |h| &h.0 as *const sys::PqvKeyFilter);
        let (k, m, np, max_np) = (k.get(), group_size.get(), nprobe.get(), max_nprobe.get());
        let mut rows = vec![0u32; nq * k * m];
        let mut dist = vec![0f32; nq * k * m];
        let mut group = vec![0i64; nq * k];
        let mut group_rows = vec![0u32; nq * k];
        let mut found = vec![0u32; nq];
        let mut used = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_grouped_expand(self.raw, group_keys.raw, keys_raw, desc_ptr, mask.map_or(ptr::null(), |x| x.raw as *const _),
                                         queries.as_ptr(), nq as u32, dim as u32, k as u32, m as u32, np as u32, max_np as u32,
                                         sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(), dist.as_mut_ptr(), group.as_mut_ptr(),
                                         group_rows.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut(), used.as_mut_ptr())
        })?;
        let hits = (0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|g| {
                        let o = (q * k + g) * m;
                        GroupSearchResult {
                            key: group[q * k + g],
                            hits: (0..group_rows[q * k + g] as usize)
                                .map(|i| SearchResult { row_idx: rows[o + i], distance: dist[o + i] })
                                .collect(),
                        }
                    })
                    .collect()
            })
            .collect();
        Ok((hits, used))
    }

    /// [`Searcher::topk_grouped`] under a per-query filter, as [`Searcher::topk_distinct_filtered`] takes it (`include/pqv.h`:
    /// `pqv_topk_grouped_filtered`).
    pub fn topk_grouped_filtered(&self, group_keys: &RowKeys, filter_keys: &RowKeys, filter: &KeyFilter, mask: Option<&RowMask>,
                                 queries: &[f32], dim: usize, k: NonZeroUsize, group_size: NonZeroUsize, nprobe: NonZeroUsize)
                                 -> Result<Vec<Vec<GroupSearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (desc, _lims, _vals) = key_filter_desc(filter, nq)?;
        let (k, m, np) = (k.get(), group_size.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k * m];
        let mut dist = vec![0f32; nq * k * m];
        let mut group = vec![0i64; nq * k];
        let mut group_rows = vec![0u32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_grouped_filtered(self.raw, group_keys.raw, filter_keys.raw, &desc, mask.map_or(ptr::null(), |x| x.raw as *const _),
                                           queries.as_ptr(), nq as u32, dim as u32, k as u32, m as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1,
                                           rows.as_mut_ptr(), dist.as_mut_ptr(), group.as_mut_ptr(), group_rows.as_mut_ptr(),
                                           found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|g| {
                        let o = (q * k + g) * m;
                        GroupSearchResult {
                            key: group[q * k + g],
                            hits: (0..group_rows[q * k + g] as usize)
                                .map(|i| SearchResult { row_idx: rows[o + i], distance: dist[o + i] })
                                .collect(),
                        }
                    })
                    .collect()
            })
            .collect())
    }

    /// Up to `group_size` rows of each of the `k` nearest groups of `keys`, groups as [`Searcher::topk_distinct`] defines them
    /// (`include/pqv.h`: `pqv_topk_grouped`).  Groups ascending by their nearest row, a group's hits by (distance, position).
    pub fn topk_grouped(&self, keys: &RowKeys, mask: Option<&RowMask>, queries: &[f32], dim: usize, k: NonZeroUsize,
                        group_size: NonZeroUsize, nprobe: NonZeroUsize) -> Result<Vec<Vec<GroupSearchResult>>> {
        let nq = if dim == 0 { 0 } else { queries.len() / dim };
        let (k, m, np) = (k.get(), group_size.get(), nprobe.get());
        let mut rows = vec![0u32; nq * k * m];
        let mut dist = vec![0f32; nq * k * m];
        let mut group = vec![0i64; nq * k];
        let mut group_rows = vec![0u32; nq * k];
        let mut found = vec![0u32; nq];
        check(unsafe {
            sys::pqv_topk_grouped(self.raw, keys.raw, mask.map_or(ptr::null(), |x| x.raw as *const _), queries.as_ptr(), nq as u32,
                                  dim as u32, k as u32, m as u32, np as u32, 0, sys::PQV_L2SQ_REF4, 1, rows.as_mut_ptr(),
                                  dist.as_mut_ptr(), group.as_mut_ptr(), group_rows.as_mut_ptr(), found.as_mut_ptr(), ptr::null_mut())
        })?;
        Ok((0..nq)
            .map(|q| {
                (0..found[q] as usize)
                    .map(|g| {
                        let o = (q * k + g) * m;
                        GroupSearchResult {
                            key: group[q * k + g],
                            hits: (0..group_rows[q * k + g] as usize)
                                .map(|i| SearchResult { row_idx: rows[o + i], distance: dist[o + i] })
                                .collect(),
                        }
                    })
                    .collect()
            })
            .collect())
    }

    /// [`Searcher::topk_grouped`] on device buffers, enqueued on `hip_stream` (NULL: the searcher's): `d_row_idx` u32 / `d_dist` f32
    /// `[nq, k, group_size]`, `d_group_key` i64 / `d_group_rows` u32 `[nq, k]`, `d_n_found` u32 / `d_n_candidates` u64 `[nq]`; the last
    /// four may be NULL.  Serves `k * group_size <= 1024`.
    ///
    /// # Safety
    /// Every non-NULL pointer must be a device allocation of at least the size above, valid until the stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn topk_grouped_device(&self, keys: &RowKeys, mask: Option<&RowMask>, d_queries: *const c_void, nq: u32, k: NonZeroUsize,
                                      group_size: NonZeroUsize, nprobe: NonZeroUsize, d_row_idx: *mut c_void, d_dist: *mut c_void,
                                      d_group_key: *mut c_void, d_group_rows: *mut c_void, d_n_found: *mut c_void,
                                      d_n_candidates: *mut c_void, hip_stream: *mut c_void) -> Result<()> {
        check(sys::pqv_topk_grouped_device(self.raw, keys.raw, mask.map_or(ptr::null(), |x| x.raw as *const _), d_queries, nq,
                                           k.get() as u32, group_size.get() as u32, nprobe.get() as u32, 0, sys::PQV_L2SQ_REF4, 1,
                                           d_row_idx, d_dist, d_group_key, d_group_rows, d_n_found, d_n_candidates, hip_stream))
    }

    /// [`Searcher::topk_distinct`] on device buffers, enqueued on `hip_stream` (NULL: the searcher's): `d_queries` f32 `[nq, dim]`,
    /// `d_row_idx` u32 / `d_dist` f32 / `d_group_key` i64 `[nq, k]`, `d_n_found` u32 / `d_n_candidates` u64 `[nq]`; the last three may
    /// be NULL.
    ///
    /// # Safety
    /// Every non-NULL pointer must be a device allocation of at least the size above, valid until the stream has run the call.
    #[allow(clippy::too_many_arguments)]
    pub unsafe fn topk_distinct_device(&self, keys: &RowKeys, mask: Option<&RowMask>, d_queries: *const c_void, nq: u32, k: NonZeroUsize,
                                       nprobe: NonZeroUsize, d_row_idx: *mut c_void, d_dist: *mut c_void, d_group_key: *mut c_void,
                                       d_n_found: *mut c_void, d_n_candidates: *mut c_void, hip_stream: *mut c_void) -> Result<()> {
        check(sys::pqv_topk_distinct_device(self.raw, keys.raw, mask.map_or(ptr::null(), |m| m.raw as *const _), d_queries, nq,
                                            k.get() as u32, nprobe.get() as u32, 0, sys::PQV_L2SQ_REF4, 1, d_row_idx, d_dist,
                                            d_group_key, d_n_found, d_n_candidates, hip_stream))
    }

    /// Plan metrics (`src/df_vector/index_exec.rs:289-299`, `exec.rs:411-427`).
    pub fn counters(&self) -> Result<sys::PqvCounters> {
        let mut c = sys::PqvCounters::default();
        check(unsafe { sys::pqv_counters(self.raw, &mut c) })?;
        Ok(c)
    }
}

impl Drop for Searcher<'_> {
    fn drop(&mut self) {
        unsafe { sys::pqv_searcher_free(self.raw) }
    }
}

/// One allow bit per row of a searcher's corpus ([`Searcher::row_mask`]); immutable, usable from any thread, and safe to drop
/// before or after its searcher.
pub struct RowMask {
    raw: *mut sys::PqvRowMask,
}
unsafe impl Send for RowMask {}
unsafe impl Sync for RowMask {}

impl RowMask {
    pub fn rows(&self) -> u64 { unsafe { sys::pqv_row_mask_rows(self.raw) } }
    /// allowed rows (that belong to an inverted list)
    pub fn count(&self) -> u64 { unsafe { sys::pqv_row_mask_count(self.raw) } }

    /// The mask of a predicate evaluated on the GPU over resident columns (`include/pqv.h`: `pqv_row_mask_from_predicates`).
    /// Leaf `i` is `(columns[i], ops[i], operands[2 i], operands[2 i + 1])` -- `masks[i]` instead of a column for a
    /// `PQV_OP_MASK` leaf -- and `program` the postfix bytes over the leaves.  Only the leaf table crosses PCIe.
    pub fn from_predicates(searcher: &Searcher, columns: &[Option<&Column>], masks: &[Option<&RowMask>], ops: &[u32],
                           operands: &[u64], program: &[u8]) -> Result<RowMask> {
        let n = ops.len();
        if columns.len() != n || masks.len() != n || operands.len() != 2 * n {
            return Err("one column slot, one mask slot and two operands per leaf".into());
        }
        let mut cols: Vec<*const sys::PqvColumn> = columns.iter().map(|c| c.map_or(ptr::null(), |c| c.raw as *const _)).collect();
        let mut ms: Vec<*const sys::PqvRowMask> = masks.iter().map(|m| m.map_or(ptr::null(), |m| m.raw as *const _)).collect();
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::pqv_row_mask_from_predicates(searcher.raw, n as u32, cols.as_mut_ptr(), ms.as_mut_ptr(), ops.as_ptr(), operands.as_ptr(),
                                              program.as_ptr(), program.len() as u32, ptr::null_mut(), &mut raw)
        })?;
        Ok(RowMask { raw })
    }

    /// One byte per corpus row: 1 where the row is allowed.
    pub fn to_bytes(&self) -> Result<Vec<u8>> {
        let mut out = vec![0u8; self.rows() as usize];
        check(unsafe { sys::pqv_row_mask_to_bytes(self.raw, out.as_mut_ptr(), out.len() as u64) })?;
        Ok(out)
    }
}

/// A scalar column resident on one GPU beside the embedding column (`include/pqv.h`: `pqv_column`): what predicate leaves read.
pub struct Column {
    raw: *mut sys::PqvColumn,
}
unsafe impl Send for Column {}
unsafe impl Sync for Column {}

impl Column {
    fn upload(device: i32, dtype: i32, values: *const c_void, valid: Option<&[u8]>, n: usize) -> Result<Column> {
        if let Some(v) = valid {
            if v.len() != n {
                return Err("one validity byte per value".into());
            }
        }
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_column_upload(device, dtype, values, valid.map_or(ptr::null(), |v| v.as_ptr()), n as u64, &mut raw) })?;
        Ok(Column { raw })
    }
    /// `valid[r] == 0` marks row `r` NULL.
    pub fn from_i32(device: i32, values: &[i32], valid: Option<&[u8]>) -> Result<Column> {
        Self::upload(device, sys::PQV_COL_I32, values.as_ptr() as *const _, valid, values.len())
    }
    pub fn from_i64(device: i32, values: &[i64], valid: Option<&[u8]>) -> Result<Column> {
        Self::upload(device, sys::PQV_COL_I64, values.as_ptr() as *const _, valid, values.len())
    }
    pub fn from_f32(device: i32, values: &[f32], valid: Option<&[u8]>) -> Result<Column> {
        Self::upload(device, sys::PQV_COL_F32, values.as_ptr() as *const _, valid, values.len())
    }
    pub fn from_f64(device: i32, values: &[f64], valid: Option<&[u8]>) -> Result<Column> {
        Self::upload(device, sys::PQV_COL_F64, values.as_ptr() as *const _, valid, values.len())
    }
    pub fn rows(&self) -> u64 { unsafe { sys::pqv_column_rows(self.raw) } }
    pub fn dtype(&self) -> i32 { unsafe { sys::pqv_column_dtype(self.raw) } }
    pub fn device(&self) -> i32 { unsafe { sys::pqv_column_device(self.raw) } }
}

impl Drop for Column {
    fn drop(&mut self) {
        unsafe { sys::pqv_column_free(self.raw) }
    }
}

impl Drop for RowMask {
    fn drop(&mut self) {
        unsafe { sys::pqv_row_mask_free(self.raw) }
    }
}

/// A key column laid out for one searcher ([`Searcher::row_keys`]): what [`Searcher::topk_keyed`] compares each query's key
/// against.  Immutable, usable from any thread, and safe to drop before or after its searcher.
pub struct RowKeys {
    raw: *mut sys::PqvRowKeys,
}
unsafe impl Send for RowKeys {}
unsafe impl Sync for RowKeys {}

impl RowKeys {
    pub fn rows(&self) -> u64 { unsafe { sys::pqv_row_keys_rows(self.raw) } }
    /// `PQV_COL_I32` or `PQV_COL_I64`
    pub fn dtype(&self) -> i32 { unsafe { sys::pqv_row_keys_dtype(self.raw) } }
}

/// A posting list per key value over one searcher's rows ([`Searcher::key_partition`]): what [`Searcher::topk_partition`] answers
/// from.  Immutable, usable from any thread, and safe to drop before or after its searcher.
pub struct KeyPartition {
    raw: *mut sys::PqvKeyPartition,
}
unsafe impl Send for KeyPartition {}
unsafe impl Sync for KeyPartition {}

impl KeyPartition {
    /// indexed rows with a valid key
    pub fn rows(&self) -> u64 { unsafe { sys::pqv_key_partition_rows(self.raw) } }
    /// distinct key values among them
    pub fn n_keys(&self) -> u64 { unsafe { sys::pqv_key_partition_n_keys(self.raw) } }
    /// `PQV_COL_I32` or `PQV_COL_I64`
    pub fn dtype(&self) -> i32 { unsafe { sys::pqv_key_partition_dtype(self.raw) } }
    /// the distinct key values ascending and their row counts
    pub fn keys(&self) -> Result<(Vec<i64>, Vec<u64>)> {
        let n = self.n_keys();
        let mut keys = vec![0i64; n as usize];
        let mut counts = vec![0u64; n as usize];
        check(unsafe { sys::pqv_key_partition_keys(self.raw, keys.as_mut_ptr(), counts.as_mut_ptr(), n) })?;
        Ok((keys, counts))
    }
}

impl Drop for KeyPartition {
    fn drop(&mut self) {
        unsafe { sys::pqv_key_partition_free(self.raw) }
    }
}

/// Where the probe depths of a [`Searcher::topk_depth`] call come from (`include/pqv.h`: `pqv_probe_depth`).
pub enum ProbeDepth {
    /// one depth per query; clamped into `[nprobe, max_nprobe]`
    Given(Vec<u32>),
    /// the lists whose centroid distance is at most this factor (squared scale, `>= 1`, may be infinite) times the nearest one's
    Ratio(f32),
}

/// One filter per query of a [`Searcher::topk_filtered`] call, compared in i64 against the key column (`include/pqv.h`:
/// `pqv_key_filter`): a key, an inclusive range (`lo > hi` matches nothing), or a set (empty: matches nothing).
pub enum KeyFilter {
    Eq(Vec<i64>),
    Range(Vec<i64>, Vec<i64>),
    In(Vec<Vec<i64>>),
}

impl Drop for RowKeys {
    fn drop(&mut self) {
        unsafe { sys::pqv_row_keys_free(self.raw) }
    }
}

/// A table of indexed files on one GPU (`src/df_vector/index_exec.rs:85-164`, one heap over the files' candidates as
/// `exec.rs:264-267`): file `f`'s rows are corpus rows `row_base[f] ..` (its index' row ids are local to the file).  It
/// derefs to a [`Searcher`] on which `nprobe` counts per file and rows come back as corpus rows; [`TableSearcher::split_row`]
/// maps one back to (file, row in that file).
pub struct TableSearcher<'c> {
    inner: Searcher<'c>,
    row_base: Vec<u64>,
    extent: Vec<u64>,
}

impl<'c> TableSearcher<'c> {
    pub fn new(indexes: &[&Index], row_base: &[u64], corpus: &'c mut Corpus) -> Result<Self> {
        Self::with_flags(indexes, row_base, corpus, sys::PQV_LAYOUT_IVF_ORDERED)
    }

    /// As [`TableSearcher::new`] with creation flags: `sys::PQV_TABLE_CAP_ROUND_ROBIN` makes `max_candidates` the reference's
    /// round-robin cap over the files (`VectorTopKOptions::max_candidates`, exec.rs:207-245) instead of an error.
    pub fn with_flags(indexes: &[&Index], row_base: &[u64], corpus: &'c mut Corpus, flags: u32) -> Result<Self> {
        if indexes.len() != row_base.len() {
            return Err("row_base needs one entry per indexed file".into());
        }
        let mut ptrs: Vec<*const sys::PqvIndex> = indexes.iter().map(|i| i.raw as *const sys::PqvIndex).collect();
        let mut raw = ptr::null_mut();
        check(unsafe {
            sys::pqv_table_searcher_create(ptrs.as_mut_ptr(), ptrs.len() as u32, row_base.as_ptr(), corpus.raw, flags, &mut raw)
        })?;
        // a file's extent is its index' row bound: after a remove the ids run past the count of list rows
        let extent = indexes.iter().map(|i| unsafe { sys::pqv_index_row_bound(i.raw) }).collect();
        Ok(Self { inner: Searcher { raw, _corpus: std::marker::PhantomData }, row_base: row_base.to_vec(), extent })
    }

    /// A corpus row of this table -> (file, row in that file); `None` outside every file.
    pub fn split_row(&self, row: u32) -> Option<(usize, u32)> {
        let r = row as u64;
        let f = self.row_base.partition_point(|&b| b <= r).checked_sub(1)?;
        let local = r - self.row_base[f];
        if row == u32::MAX || local >= self.extent[f] { None } else { Some((f, local as u32)) }
    }
}

/// What `CandidateCursor::next_batch(max_candidates)` of a fresh cursor takes from each file (access.rs:214-242), from the
/// files' candidate counts alone; `max_candidates == 0`: no cap.  The quotas of a round-robin capped [`TableSearcher`].
pub fn round_robin_quota(counts: &[u64], max_candidates: u64) -> Result<Vec<u64>> {
    let mut quota = vec![0u64; counts.len()];
    check(unsafe { sys::pqv_round_robin_quota(counts.as_ptr(), u32::try_from(counts.len())?, max_candidates, quota.as_mut_ptr()) })?;
    Ok(quota)
}

impl<'c> std::ops::Deref for TableSearcher<'c> {
    type Target = Searcher<'c>;
    fn deref(&self) -> &Searcher<'c> {
        &self.inner
    }
}

/// `TopkBuilder` (`src/ivf/search.rs:49-81`) over a cached [`Searcher`] instead of a path.
pub struct TopkBuilder<'a, 'c> {
    searcher: &'a Searcher<'c>,
    query: &'a [f32],
    k: Option<NonZeroUsize>,
    nprobe: Option<NonZeroUsize>,
}

impl<'a, 'c> TopkBuilder<'a, 'c> {
    pub fn new(searcher: &'a Searcher<'c>, query: &'a [f32]) -> Self {
        Self { searcher, query, k: None, nprobe: None }
    }
    pub fn k(mut self, k: usize) -> Result<Self> {
        self.k = Some(NonZeroUsize::new(k).ok_or("k must be > 0")?); // search.rs:67
        Ok(self)
    }
    pub fn nprobe(mut self, nprobe: usize) -> Result<Self> {
        self.nprobe = Some(NonZeroUsize::new(nprobe).ok_or("nprobe must be > 0")?); // search.rs:72
        Ok(self)
    }
    /// Blocking (the reference's `async fn search` runs its CPU loop inline as well, `search.rs:112-127`).
    pub fn search(self) -> Result<Vec<SearchResult>> {
        let k = self.k.ok_or("k must be set")?; // search.rs:77
        let nprobe = self.nprobe.ok_or("nprobe must be set")?; // search.rs:78
        Ok(self.searcher.topk(self.query, self.query.len(), k, nprobe)?.pop().unwrap_or_default())
    }
}

/// The running top-k of `VectorTopKExec::topk_from_batches` (`src/df_vector/exec.rs:257-277`): fold one
/// `RecordBatch` at a time, materialise `ScalarValue`s only for the <= k survivors at the end.  `rows` / `d2` hold
/// the reference `BinaryHeap`'s backing array between batches (the library replays `push` / `peek` / `pop` exactly,
/// so ties come out as in the reference).
pub struct RerankState {
    device: usize,
    k: usize,
    rows: Vec<u32>,
    d2: Vec<f32>,
    count: u32,
}

impl RerankState {
    pub fn new(device: usize, k: usize) -> Self {
        Self { device, k, rows: vec![0; k.max(1)], d2: vec![0.0; k.max(1)], count: 0 }
    }

    fn check_lens(m: usize, ids: Option<&[u32]>, valid: Option<&[u8]>) -> Result<()> {
        if ids.map_or(false, |v| v.len() != m) { return Err("ids length must equal the number of rows".into()); }
        if valid.map_or(false, |v| v.len() != m) { return Err("valid length must equal the number of rows".into()); }
        Ok(())
    }

    /// `values`: the batch's list-values buffer `[m, dim]`; `ids`: the payload per row (e.g. batch-global row
    /// numbers; `None` = 0..m); `valid`: 0 for null rows / wrong-length lists (`exec.rs:496-498,526-528`).
    /// Distances use the element-by-element order of `compute_distance_values` (`exec.rs:529-533`).
    pub fn fold_batch(&mut self, query: &[f32], values: &[f32], ids: Option<&[u32]>, valid: Option<&[u8]>) -> Result<()> {
        let dim = query.len();
        let m = if dim == 0 { 0 } else { values.len() / dim };
        Self::check_lens(m, ids, valid)?;
        check(unsafe {
            sys::pqv_rerank(self.device as c_int, query.as_ptr(), values.as_ptr(), ids.map_or(ptr::null(), |v| v.as_ptr()),
                            valid.map_or(ptr::null(), |v| v.as_ptr()), m as u64, dim as u32, self.k as u32,
                            sys::PQV_L2SQ_SEQ, self.rows.as_mut_ptr(), self.d2.as_mut_ptr(), &mut self.count)
        })
    }

    /// The same for a `Float64Array` values buffer: each value is narrowed `as f32` first (`exec.rs:538-545`).
    pub fn fold_batch_f64(&mut self, query: &[f32], values: &[f64], ids: Option<&[u32]>, valid: Option<&[u8]>) -> Result<()> {
        let dim = query.len();
        let m = if dim == 0 { 0 } else { values.len() / dim };
        Self::check_lens(m, ids, valid)?;
        check(unsafe {
            sys::pqv_rerank_f64(self.device as c_int, query.as_ptr(), values.as_ptr(), ids.map_or(ptr::null(), |v| v.as_ptr()),
                                valid.map_or(ptr::null(), |v| v.as_ptr()), m as u64, dim as u32, self.k as u32,
                                sys::PQV_L2SQ_SEQ, self.rows.as_mut_ptr(), self.d2.as_mut_ptr(), &mut self.count)
        })
    }

    /// (payload, squared distance) in output order: `heap.into_iter()` + the stable sort of `exec.rs:269-274`
    /// (no distance column, no sqrt on this path).
    pub fn finish(self) -> Result<Vec<(u32, f32)>> {
        let n = self.count as usize;
        let mut rows = vec![0u32; n.max(1)];
        let mut d2 = vec![0f32; n.max(1)];
        check(unsafe { sys::pqv_rerank_finish(self.rows.as_ptr(), self.d2.as_ptr(), self.count, rows.as_mut_ptr(), d2.as_mut_ptr()) })?;
        Ok((0..n).map(|i| (rows[i], d2[i])).collect())
    }
}

/// One rank of the sharded search (`src/df_vector/index_exec.rs:85-164` probes every file's own index;
/// `src/df_vector/exec.rs:264-267` merges them in one heap): one process per GPU, each holding a row range and its
/// index; `exchange` is ONE RCCL all-gather of the per-shard top-k + the deterministic merge, no torch involved.
pub struct ShardComm {
    raw: *mut sys::PqvShardComm,
}
unsafe impl Send for ShardComm {}

impl ShardComm {
    /// Rank 0 draws the rendezvous id and distributes the 128 bytes over the host's own channel.
    pub fn unique_id() -> Result<[u8; 128]> {
        let mut id = [0u8; 128];
        check(unsafe { sys::pqv_shard_unique_id(id.as_mut_ptr()) })?;
        Ok(id)
    }
    /// Collective over all ranks.
    pub fn new(device: usize, rank: u32, world: u32, id: &[u8; 128]) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_shard_comm_create(device as c_int, rank, world, id.as_ptr(), &mut raw) })?;
        Ok(Self { raw })
    }
    pub fn rank(&self) -> u32 { unsafe { sys::pqv_shard_comm_rank(self.raw) } }
    pub fn world(&self) -> u32 { unsafe { sys::pqv_shard_comm_world(self.raw) } }
    /// Device pointers: this rank's `pqv_topk_device` outputs `[nq, k]`, the shards' first global rows `i64[world]`,
    /// outputs `f32 / i64 [nq, k]` -- identical on every rank.  Asynchronous on `hip_stream`.
    ///
    /// # Safety
    /// All pointers must be valid device allocations of the stated sizes on this communicator's GPU.
    pub unsafe fn exchange(&mut self, d_dist: *const c_void, d_rows: *const c_void, d_row_base: *const c_void, nq: u32, k: u32,
                           d_out_dist: *mut c_void, d_out_rows: *mut c_void, hip_stream: *mut c_void) -> Result<()> {
        check(sys::pqv_shard_exchange(self.raw, d_dist, d_rows, d_row_base, nq, k, d_out_dist, d_out_rows, hip_stream))
    }
}

impl Drop for ShardComm {
    fn drop(&mut self) {
        unsafe { sys::pqv_shard_comm_free(self.raw) }
    }
}

/// `CandidateCursor` (`src/df_vector/access.rs:193-243`).
pub struct CandidateCursor {
    raw: *mut sys::PqvCandidateCursor,
    files: usize,
}

impl CandidateCursor {
    pub fn new(file_count: usize) -> Result<Self> {
        let mut raw = ptr::null_mut();
        check(unsafe { sys::pqv_candidate_cursor_new(file_count as u32, &mut raw) })?;
        Ok(Self { raw, files: file_count })
    }
    pub fn add_candidates(&mut self, idx: usize, candidates: &[u32]) -> Result<()> {
        check(unsafe { sys::pqv_candidate_cursor_add(self.raw, idx as u32, candidates.as_ptr(), candidates.len() as u64) })
    }
    pub fn next_batch(&mut self, batch_size: usize) -> Result<Vec<(usize, u32)>> {
        let mut files = vec![0u32; batch_size.max(1)];
        let mut rows = vec![0u32; batch_size.max(1)];
        let mut n = 0u64;
        let mut taken = vec![0u64; self.files.max(1)];
        check(unsafe {
            sys::pqv_candidate_cursor_next_batch(self.raw, batch_size as u64, files.as_mut_ptr(), rows.as_mut_ptr(), &mut n, taken.as_mut_ptr())
        })?;
        Ok((0..n as usize).map(|i| (files[i] as usize, rows[i])).collect())
    }
}

impl Drop for CandidateCursor {
    fn drop(&mut self) {
        unsafe { sys::pqv_candidate_cursor_free(self.raw) }
    }
}

/// The `(lims, rows)` arrays of a candidate-list call: one list per query, concatenated in order.
fn candidate_lists(candidates: &[Vec<u32>], nq: usize) -> Result<(Vec<u64>, Vec<u32>)> {
    if candidates.len() != nq {
        return Err("one candidate list per query".into());
    }
    let mut lims = Vec::with_capacity(nq + 1);
    lims.push(0u64);
    let mut rows = Vec::with_capacity(candidates.iter().map(Vec::len).sum());
    for c in candidates {
        rows.extend_from_slice(c);
        lims.push(rows.len() as u64);
    }
    Ok((lims, rows))
}

/// The C descriptor of a [`KeyFilter`] for `nq` queries, with the arrays it points at (a set filter's offsets and sorted,
/// de-duplicated values): they must outlive the call that reads the descriptor.
fn key_filter_desc(filter: &KeyFilter, nq: usize) -> Result<(sys::PqvKeyFilter, Vec<u64>, Vec<i64>)> {
    match filter {
        KeyFilter::Eq(a) => {
            if a.len() != nq {
                return Err("one query key per query".into());
            }
            Ok((sys::PqvKeyFilter { kind: sys::PQV_KEY_EQ, reserved: 0, a: a.as_ptr() as *const c_void, b: ptr::null() }, Vec::new(), Vec::new()))
        }
        KeyFilter::Range(lo, hi) => {
            if lo.len() != nq || hi.len() != nq {
                return Err("one lower and one upper bound per query".into());
            }
            Ok((sys::PqvKeyFilter { kind: sys::PQV_KEY_RANGE, reserved: 0, a: lo.as_ptr() as *const c_void, b: hi.as_ptr() as *const c_void },
                Vec::new(), Vec::new()))
        }
        KeyFilter::In(sets) => {
            if sets.len() != nq {
                return Err("one query key set per query".into());
            }
            let mut lims = vec![0u64; nq + 1];
            let mut vals: Vec<i64> = Vec::new();
            for (q, set) in sets.iter().enumerate() {
                let mut s = set.clone();
                s.sort_unstable();
                s.dedup();
                if s.len() > sys::PQV_KEY_SET_MAX {
                    return Err("a query key set takes at most 1024 values".into());
                }
                vals.extend_from_slice(&s);
                lims[q + 1] = vals.len() as u64;
            }
            if vals.is_empty() {
                vals.push(0); // (never read: a readable address for the descriptor)
            }
            // (moving the vectors out does not move their heap buffers: the descriptor's pointers stay valid)
            let desc = sys::PqvKeyFilter { kind: sys::PQV_KEY_IN, reserved: 0, a: lims.as_ptr() as *const c_void, b: vals.as_ptr() as *const c_void };
            Ok((desc, lims, vals))
        }
    }
}
