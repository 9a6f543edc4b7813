"""Host-side mirror of the reference's builder API over the C ABI (include/pqv.h).

Names, argument meaning and error texts follow src/ivf/parquet.rs:23-103 (IndexBuilder),
src/ivf/search.rs:41-81 (TopkBuilder, SearchResult) and src/ivf/index.rs:9-14 (IvfIndex).
"""
import ctypes as C
from dataclasses import dataclass

import numpy as np

from . import _ffi, predicate
from ._ffi import f32p, f64p, u8p, u32p, u64p, vp


class PqvError(Exception):
    """Carries the library's status code and the reference's message text."""

    def __init__(self, code, message):
        super().__init__(message)
        self.code = code
        self.message = message


def _check(rc):
    if rc != _ffi.PQV_OK:
        raise PqvError(rc, _ffi.lib().pqv_last_error().decode())


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def device_count():
    return _ffi.lib().pqv_device_count()


# ---------------------------------------------------------------------------------------
class Corpus:
    """The embedding column resident in one GPU's HBM (row-major [n, dim] f32)."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keepalive = keepalive

    @classmethod
    def upload(cls, rows, device=0):
        rows = np.asarray(rows)
        if rows.ndim != 2:
            raise PqvError(_ffi.PQV_ERR_INVALID, "Embedding data length must be a multiple of dimension")
        n, dim = rows.shape
        h = vp()
        if rows.dtype == np.float64:  # narrowed like src/ivf/parquet.rs:246-256
            _check(_ffi.lib().pqv_corpus_create(device, n, dim, C.byref(h)))
            c = cls(h)
            r64 = np.ascontiguousarray(rows)
            _check(_ffi.lib().pqv_corpus_append_f64(h, r64.ctypes.data_as(f64p), n))
            return c
        r = _f32(rows)
        _check(_ffi.lib().pqv_corpus_upload(device, r.ctypes.data_as(f32p), n, dim, C.byref(h)))
        return cls(h)

    @classmethod
    def create(cls, capacity_rows, dim, device=0):
        h = vp()
        _check(_ffi.lib().pqv_corpus_create(device, capacity_rows, dim, C.byref(h)))
        c = cls(h)
        c._capacity = int(capacity_rows)
        return c

    @property
    def capacity(self):
        """Rows the corpus has room for (Corpus.create's capacity_rows; else its row count)."""
        return getattr(self, "_capacity", None) or self.rows

    def append(self, rows):
        rows = np.asarray(rows)
        if rows.dtype == np.float64:
            r = np.ascontiguousarray(rows)
            _check(_ffi.lib().pqv_corpus_append_f64(self._h, r.ctypes.data_as(f64p), r.shape[0]))
        else:
            r = _f32(rows)
            _check(_ffi.lib().pqv_corpus_append(self._h, r.ctypes.data_as(f32p), r.shape[0]))

    def write_rows(self, row_offset, rows):
        """Streaming upload (pqv_corpus_write_rows): rows [row_offset, row_offset + len(rows)) from a [m, dim] f32 / f64 array,
        staged in pinned memory and DMA'd asynchronously.  Thread-safe; batches may arrive in any order.  finish() completes."""
        rows = np.asarray(rows)
        if rows.dtype == np.float64:
            r = np.ascontiguousarray(rows)
            _check(_ffi.lib().pqv_corpus_write_rows_f64(self._h, row_offset, r.ctypes.data_as(f64p), r.shape[0]))
        else:
            r = _f32(rows)
            _check(_ffi.lib().pqv_corpus_write_rows(self._h, row_offset, r.ctypes.data_as(f32p), r.shape[0]))

    def write_rows_ptr(self, row_offset, address, n_rows, f64=False):
        """write_rows from a raw host address (a page inside a memory-mapped file: no intermediate array)."""
        fn = _ffi.lib().pqv_corpus_write_rows_f64 if f64 else _ffi.lib().pqv_corpus_write_rows
        _check(fn(self._h, row_offset, C.cast(C.c_void_p(address), f64p if f64 else f32p), n_rows))

    def write_plain_pages(self, file_base, body_off, body_len, first_value, n_values, dim, max_def, f64=False):
        """A run of uncompressed PLAIN data pages from a mapped file (pqv_corpus_write_plain_pages): level runs checked and values
        uploaded natively.  Returns None, or the index of the first page that is not what the page plan assumed."""
        bad = C.c_uint32(0)
        rc = _ffi.lib().pqv_corpus_write_plain_pages(self._h, C.cast(C.c_void_p(file_base), _ffi.u8p), body_off.ctypes.data_as(_ffi.u64p),
                                                     body_len.ctypes.data_as(_ffi.u32p), first_value.ctypes.data_as(_ffi.u64p),
                                                     n_values.ctypes.data_as(_ffi.u32p), len(body_off), dim, max_def, 1 if f64 else 0, C.byref(bad))
        if rc == 1:
            return int(bad.value)
        _check(rc)
        return None

    def finish(self, n_rows):
        _check(_ffi.lib().pqv_corpus_finish(self._h, n_rows))

    @classmethod
    def from_device_ptr(cls, ptr, n, dim, device=0, keepalive=None):
        """Adopt a device buffer (e.g. a torch tensor's data_ptr()); `keepalive` pins its owner."""
        h = vp()
        _check(_ffi.lib().pqv_corpus_from_device(device, vp(ptr), n, dim, C.byref(h)))
        return cls(h, keepalive)

    @property
    def rows(self):
        return _ffi.lib().pqv_corpus_rows(self._h)

    @property
    def dim(self):
        return _ffi.lib().pqv_corpus_dim(self._h)

    @property
    def device(self):
        return _ffi.lib().pqv_corpus_device(self._h)

    def fetch_rows(self, row_ids):
        ids = np.ascontiguousarray(row_ids, dtype=np.uint32)
        out = np.empty((ids.size, self.dim), dtype=np.float32)
        _check(_ffi.lib().pqv_corpus_fetch_rows(self._h, ids.ctypes.data_as(u32p), ids.size,
                                                out.ctypes.data_as(f32p)))
        return out

    def brute_topk(self, queries, k, metric=_ffi.PQV_COSINE):
        """Exhaustive batched top-k over every resident row on the matrix cores (extension:
        cosine / norm-expansion L2).  Returns (row_idx [nq,k], dist [nq,k], n_found [nq])."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        nf = np.zeros(nq, dtype=np.uint32)
        _check(_ffi.lib().pqv_brute_topk(self._h, q.ctypes.data_as(f32p), nq, qlen, k, metric,
                                         rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p),
                                         nf.ctypes.data_as(u32p)))
        return rows, dist, nf

    def close(self):
        if self._h:
            _ffi.lib().pqv_corpus_free(self._h)
            self._h = None
        self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------
class Index:
    """IvfIndex{dim, n_clusters, centroids, inverted_lists} (src/ivf/index.rs:9-14)."""

    def __init__(self, handle, row_bound=None):
        self._h = handle
        self._row_bound = row_bound      # largest indexed row id + 1 where it is known by construction (a build, an append)

    @classmethod
    def from_bytes(cls, blob):
        h = vp()
        blob = bytes(blob)
        _check(_ffi.lib().pqv_index_from_bytes(blob, len(blob), C.byref(h)))
        return cls(h)

    @classmethod
    def from_parts(cls, dim, centroids, lists):
        cent = _f32(centroids).reshape(-1)
        k = len(lists)
        off = np.zeros(k + 1, dtype=np.uint64)
        for i, l in enumerate(lists):
            off[i + 1] = off[i] + len(l)
        rows = (np.concatenate([np.asarray(l, dtype=np.uint32) for l in lists])
                if k and off[-1] else np.zeros(0, dtype=np.uint32))
        rows = np.ascontiguousarray(rows, dtype=np.uint32)
        h = vp()
        _check(_ffi.lib().pqv_index_from_parts(dim, k, cent.ctypes.data_as(f32p),
                                               off.ctypes.data_as(u64p), rows.ctypes.data_as(u32p),
                                               C.byref(h)))
        return cls(h)

    def to_bytes(self):
        buf = u8p()
        n = C.c_size_t(0)
        _check(_ffi.lib().pqv_index_to_bytes(self._h, C.byref(buf), C.byref(n)))
        try:
            return C.string_at(buf, n.value)
        finally:
            _ffi.lib().pqv_bytes_free(buf)

    @property
    def dim(self):
        return _ffi.lib().pqv_index_dim(self._h)

    @property
    def n_clusters(self):
        return _ffi.lib().pqv_index_n_clusters(self._h)

    @property
    def n_rows(self):
        return _ffi.lib().pqv_index_n_rows(self._h)

    @property
    def centroids(self):
        p = _ffi.lib().pqv_index_centroids(self._h)
        return np.ctypeslib.as_array(p, shape=(self.n_clusters, self.dim)).copy()

    @property
    def list_offsets(self):
        p = _ffi.lib().pqv_index_list_offsets(self._h)
        return np.ctypeslib.as_array(p, shape=(self.n_clusters + 1,)).copy()

    @property
    def list_rows(self):
        n = self.n_rows
        if n == 0:
            return np.zeros(0, dtype=np.uint32)
        p = _ffi.lib().pqv_index_list_rows(self._h)
        return np.ctypeslib.as_array(p, shape=(n,)).copy()

    def inverted_lists(self):
        off, rows = self.list_offsets, self.list_rows
        return [rows[int(off[i]):int(off[i + 1])] for i in range(self.n_clusters)]

    @property
    def row_bound(self):
        """Largest indexed row id + 1 (0 for empty lists): the first row an append may start at."""
        if self._row_bound is None:
            rows = self.list_rows
            self._row_bound = int(rows.max()) + 1 if rows.size else 0
        return self._row_bound

    def assign(self, corpus, first_row=0, n_rows=None):
        """Nearest centroid (src/ivf/index.rs:244-257) of corpus rows [first_row, first_row + n_rows) under this index'
        centroids; n_rows None = to the end of the corpus.  -> uint32 [n_rows]."""
        if n_rows is None:
            n_rows = max(corpus.rows - first_row, 0)
        out = np.empty(n_rows, dtype=np.uint32)
        _check(_ffi.lib().pqv_index_assign(self._h, corpus._h, first_row, n_rows, out.ctypes.data_as(u32p)))
        return out

    def append(self, corpus, first_row=None, n_rows=None):
        """A new Index: these centroids, every list followed by the rows of [first_row, first_row + n_rows) assigned to it,
        ascending (pqv_index_append).  first_row None = this index' row bound, n_rows None = to the end of the corpus, so
        `corpus.append(batch); index = index.append(corpus)` is the whole ingest step.  This index is not modified."""
        if first_row is None:
            first_row = self.row_bound
        if n_rows is None:
            n_rows = max(corpus.rows - first_row, 0)
        h = vp()
        _check(_ffi.lib().pqv_index_append(self._h, corpus._h, first_row, n_rows, C.byref(h)))
        return Index(h, row_bound=first_row + n_rows)

    def remove(self, rows=None, *, flags=None, where=None, device=0, stream=0):
        """A new Index: these centroids, every list without the removed rows, order kept (pqv_index_remove*).  Row ids stay what
        they were and the row bound is carried over, so a later append continues where it would have; an unmasked search of the
        result answers what a search of this index under the equivalent mask answers, through every fast path.  Exactly one of:
          rows   row ids to remove -- any order, duplicates allowed, ids that are not indexed ignored;
          flags  one byte (or bool) per row id from 0, non-zero REMOVES the row, ids beyond the array stay: a numpy array, a
                 torch tensor (on the GPU: read in place), or (device pointer, count) as row_mask_device takes them;
          where  a RowMask: the rows the mask ALLOWS are removed -- DELETE WHERE predicate, the opposite sense of passing the
                 mask to a search (read through to_bytes()).
        Runs on `device` where there is one (flags on the GPU need it), else on the host with the same result.  This index is
        not modified: searchers made from it, and their masks and keys, stay as they were."""
        if (rows is not None) + (flags is not None) + (where is not None) != 1:
            raise PqvError(_ffi.PQV_ERR_INVALID, "remove() takes exactly one of rows, flags and where")
        lib, h = _ffi.lib(), vp()
        bound = self.row_bound               # carried over, not lowered (known by construction, else one scan of the host lists)
        if rows is not None:
            r = np.ascontiguousarray(np.asarray(rows).reshape(-1), dtype=np.uint32)
            _check(lib.pqv_index_remove_rows(self._h, device, r.ctypes.data_as(u32p), r.size, C.byref(h)))
            return Index(h, row_bound=bound)
        if where is not None:
            flags = where.to_bytes()
        ptr = count = None
        if isinstance(flags, tuple):
            ptr, count = int(flags[0]), int(flags[1])
        elif hasattr(flags, "data_ptr") and getattr(flags, "is_cuda", False):
            if flags.element_size() != 1 or not flags.is_contiguous():
                raise PqvError(_ffi.PQV_ERR_INVALID, "remove flags on the device must be contiguous bytes or bools")
            ptr, count = int(flags.data_ptr()), int(flags.numel())
        if ptr is not None:
            _check(lib.pqv_index_remove_device(self._h, device, vp(ptr or None), count, vp(stream or None), C.byref(h)))
            return Index(h, row_bound=bound)
        a = flags.numpy() if hasattr(flags, "data_ptr") else np.asarray(flags)
        if a.dtype != np.bool_ and a.dtype != np.uint8:
            raise PqvError(_ffi.PQV_ERR_INVALID, "remove flags must be bool or uint8, one entry per row id")
        a = np.ascontiguousarray(a.reshape(-1)).view(np.uint8)
        _check(lib.pqv_index_remove(self._h, device, a.ctypes.data_as(u8p), a.size, C.byref(h)))
        return Index(h, row_bound=bound)

    def compact(self, corpus, capacity=None):
        """-> (Corpus, Index, old_row): a dense corpus of the rows this index still holds (ascending old id, bit for bit, room for
        max(capacity, kept) rows), this index renumbered onto it (new id = rank of the old id among the kept rows; lists keep their
        order), and old_row uint32 [kept] = the old id of every new row -- attached columns, masks and keys are re-made from
        column[old_row].  Neither this index nor `corpus` is modified (pqv_index_compact)."""
        old_row = np.zeros(max(self.n_rows, 1), dtype=np.uint32)
        ch, ih = vp(), vp()
        _check(_ffi.lib().pqv_index_compact(self._h, corpus._h, int(capacity or 0), C.byref(ch), C.byref(ih), old_row.ctypes.data_as(u32p)))
        dense = Corpus(ch)
        dense._capacity = max(int(capacity or 0), dense.rows)
        return dense, Index(ih, row_bound=dense.rows), old_row[:dense.rows].copy()

    def close(self):
        if self._h:
            _ffi.lib().pqv_index_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------
class IndexBuilder:
    """src/ivf/parquet.rs:23-103.  `source` is a Parquet path (with `embedding_column`, as in the
    reference), a Corpus or a [n, dim] array (the in-memory form of the embedding column);
    defaults n_clusters=None -> ceil(sqrt(n)), max_iters=20, seed=42 (:32-39)."""

    def __init__(self, source, embedding_column=None, device=0):
        self._source = source
        self._embedding_column = embedding_column
        self._device = device
        self._n_clusters = None
        self._max_iters = 20
        self._seed = 42
        self._workers = 0
        self._centroids = None

    def with_centroids(self, index_or_array):
        """Index the source under a given codebook: the centroids of an Index, or a [k, dim] array.  build(), build_inplace() and
        build_new() then skip k-means (max_iters, seed and workers are ignored; there is no n_clusters <= rows rule, which
        is k-means') and return Index.from_parts(dim, centroids, empty lists).append(corpus, 0, n): several files of a
        table, or several shards, can share one partition."""
        cent = index_or_array.centroids if isinstance(index_or_array, Index) else np.asarray(index_or_array)
        if cent.ndim != 2 or cent.shape[0] == 0 or cent.shape[1] == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "centroids must be a [k, dim] array with k > 0 and dim > 0")
        self._centroids = _f32(cent)
        return self

    def n_clusters(self, n_clusters):
        self._n_clusters = n_clusters
        return self

    def max_iters(self, max_iters):
        self._max_iters = max_iters
        return self

    def seed(self, seed):
        self._seed = seed
        return self

    def workers(self, workers):
        """The available_parallelism() to reproduce; 0 = this host's CPU count."""
        self._workers = workers
        return self

    def _config(self):
        # build_config, src/ivf/parquet.rs:88-102
        if self._max_iters == 0 and self._centroids is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "max_iters must be > 0")
        if self._centroids is not None and self._n_clusters not in (None, len(self._centroids)):
            raise PqvError(_ffi.PQV_ERR_INVALID, f"n_clusters {self._n_clusters} does not match the {len(self._centroids)} given centroids")
        if self._n_clusters is not None and self._n_clusters == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "n_clusters must be > 0")
        if self._embedding_column is not None and not str(self._embedding_column).strip():
            raise PqvError(_ffi.PQV_ERR_INVALID, "Embedding column name cannot be empty")
        return (self._n_clusters or 0), self._max_iters, self._seed, self._workers

    def _is_path(self):
        import os
        return isinstance(self._source, (str, bytes, os.PathLike))

    def _require_column(self):
        if not self._is_path():
            raise PqvError(_ffi.PQV_ERR_INVALID, "build_inplace/build_new need a Parquet path as source")
        if self._embedding_column is None or not str(self._embedding_column).strip():
            raise PqvError(_ffi.PQV_ERR_INVALID, "Embedding column name cannot be empty")   # mod.rs:25

    def _build_on(self, corpus):
        nc, mi, seed, workers = self._config()
        if self._centroids is not None:
            k, dim = self._centroids.shape
            empty = Index.from_parts(dim, self._centroids, [np.zeros(0, np.uint32)] * k)
            return empty.append(corpus, 0, corpus.rows)
        h = vp()
        _check(_ffi.lib().pqv_index_build(corpus._h, nc, mi, seed, workers, C.byref(h)))
        return Index(h, row_bound=corpus.rows)

    def _load_parquet(self):
        from . import parquet_io
        self._config()                       # build_config() runs first (parquet.rs:58,72)
        self._require_column()
        self.last_stats = {"load": {}}
        return parquet_io.load_embedding_column(self._source, self._embedding_column, self._device, stats=self.last_stats["load"])

    def _timed_build(self, write):
        """load -> build -> write, with the wall time of each in self.last_stats (the reference's benches/index_build.rs times
        the three together)."""
        import time
        t0 = time.perf_counter()
        corpus = self._load_parquet()
        t1 = time.perf_counter()
        index = self._build_on(corpus)
        t2 = time.perf_counter()
        write(index)
        t3 = time.perf_counter()
        self.last_stats.update({"load_s": t1 - t0, "build_s": t2 - t1, "write_s": t3 - t2, "total_s": t3 - t0})
        corpus.close()
        return index

    def build_inplace(self):
        """Build and append the index to the source file (src/ivf/parquet.rs:57-69)."""
        from . import parquet_io
        return self._timed_build(lambda index: parquet_io.append_index_inplace(self._source, index, self._embedding_column))

    def build_new(self, output):
        """Build and write a new file that carries the index (src/ivf/parquet.rs:71-86)."""
        from . import parquet_io
        return self._timed_build(lambda index: parquet_io.write_parquet_with_index(self._source, output, index, self._embedding_column))

    def build(self):
        """In-memory form: returns the Index without touching any file."""
        nc, mi, seed, workers = self._config()
        if self._is_path():
            return self._build_on(self._load_parquet())
        if isinstance(self._source, Corpus):
            return self._build_on(self._source)
        data = np.asarray(self._source)
        if data.ndim != 2:
            raise PqvError(_ffi.PQV_ERR_INVALID, "Embedding data length must be a multiple of dimension")
        if self._centroids is not None:
            return self._build_on(Corpus.upload(data, device=self._device))
        dim = data.shape[1]
        flat = _f32(data).reshape(-1)
        h = vp()
        _check(_ffi.lib().pqv_index_build_host(self._device, flat.ctypes.data_as(f32p), flat.size,
                                               dim, nc, mi, seed, workers, C.byref(h)))
        return Index(h)


# ---------------------------------------------------------------------------------------
class CandidateCursor:
    """src/df_vector/access.rs:193-243: round-robin over per-file candidate lists until a cap."""

    def __init__(self, file_count):
        h = vp()
        _check(_ffi.lib().pqv_candidate_cursor_new(file_count, C.byref(h)))
        self._h = h
        self.file_count = file_count

    def add_candidates(self, idx, rows):
        r = np.ascontiguousarray(rows, dtype=np.uint32)
        _check(_ffi.lib().pqv_candidate_cursor_add(self._h, idx, r.ctypes.data_as(u32p), r.size))

    def next_batch(self, batch_size):
        """Returns ([(file_idx, row), ...], cumulative rows taken per file)."""
        of = np.zeros(max(1, batch_size), dtype=np.uint32)
        orow = np.zeros(max(1, batch_size), dtype=np.uint32)
        n = C.c_uint64(0)
        taken = np.zeros(max(1, self.file_count), dtype=np.uint64)
        _check(_ffi.lib().pqv_candidate_cursor_next_batch(self._h, batch_size, of.ctypes.data_as(u32p), orow.ctypes.data_as(u32p),
                                                         C.byref(n), taken.ctypes.data_as(u64p)))
        return list(zip(of[:n.value].tolist(), orow[:n.value].tolist())), taken[:self.file_count].copy()

    def __del__(self):
        try:
            if self._h:
                _ffi.lib().pqv_candidate_cursor_free(self._h)
                self._h = None
        except Exception:
            pass


# ---------------------------------------------------------------------------------------
@dataclass
class SearchResult:
    """src/ivf/search.rs:41-45"""
    row_idx: int
    distance: float


@dataclass
class DistinctSearchResult:
    """One group of a distinct top-k (TopkBuilder.distinct_on): the group's nearest row, its distance, the group's key value."""
    row_idx: int
    distance: float
    key: int


@dataclass
class GroupSearchResult:
    """One group of a grouped top-k (TopkBuilder.distinct_on(..).group_size(m)): the group's key value and its up to m nearest rows,
    nearest first -- [SearchResult], or [TableSearchResult] from a TableTopkBuilder."""
    key: int
    hits: list


_COLUMN_DTYPES = {np.dtype(np.int32): _ffi.PQV_COL_I32, np.dtype(np.int64): _ffi.PQV_COL_I64,
                  np.dtype(np.float32): _ffi.PQV_COL_F32, np.dtype(np.float64): _ffi.PQV_COL_F64}
_RESIDENT_TYPES = "int8..int64, uint8..uint32, bool, date, timestamp, time64, float, double"


def _arrow_scalar_target(typ):
    """The resident type (a pyarrow type) of an Arrow column type, or None where the column cannot be resident."""
    import pyarrow as pa
    ty = pa.types
    if ty.is_boolean(typ) or ty.is_int8(typ) or ty.is_int16(typ) or ty.is_int32(typ) or ty.is_uint8(typ) or ty.is_uint16(typ) \
            or ty.is_date32(typ):
        return pa.int32()
    if ty.is_int64(typ) or ty.is_uint32(typ) or ty.is_date64(typ) or ty.is_timestamp(typ) or ty.is_time64(typ):
        return pa.int64()
    if ty.is_float32(typ):
        return pa.float32()
    if ty.is_float64(typ):
        return pa.float64()
    return None


def scalar_arrays(values, valid=None, name=None):
    """-> (values, valid or None, PQV_COL_*): contiguous numpy values of a resident type and validity bytes (0 = NULL) from a
    numpy array (int32 / int64 / float32 / float64, plus an optional bool / uint8 `valid`) or a pyarrow Array / ChunkedArray, whose
    nulls become validity bytes (int8 / int16 / uint8 / uint16 / bool / date32 -> int32; uint32 / date64 / timestamp / time64 ->
    int64).  Anything else is refused."""
    what = f"column {name!r}" if name else "the column"
    if not isinstance(values, np.ndarray) and hasattr(values, "type") and hasattr(values, "null_count"):
        import pyarrow as pa
        import pyarrow.compute as pc
        arr = values.combine_chunks() if isinstance(values, pa.ChunkedArray) else values
        target = _arrow_scalar_target(arr.type)
        if target is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} has type {arr.type}: not a resident scalar type ({_RESIDENT_TYPES}); "
                                                 "filter on it on the host with a pyarrow expression (pyarrow.compute.field(...))")
        if valid is not None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "valid= goes with numpy values; a pyarrow array carries its own nulls")
        if arr.null_count:
            valid = pc.is_valid(arr).to_numpy(zero_copy_only=False).astype(np.uint8)
        if pa.types.is_boolean(arr.type):
            arr = arr.cast(pa.int8())
        elif pa.types.is_date64(arr.type) or pa.types.is_timestamp(arr.type) or pa.types.is_time64(arr.type):
            arr = arr.cast(pa.int64())
        elif pa.types.is_date32(arr.type):
            arr = arr.cast(pa.int32())
        arr = arr.cast(target)
        if arr.null_count:
            arr = pc.fill_null(arr, pa.scalar(0, type=target))
        values = arr.to_numpy(zero_copy_only=False)
    a = np.asarray(values)
    if a.ndim != 1:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} must be one-dimensional, got {a.ndim} dimensions")
    if a.dtype not in _COLUMN_DTYPES:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} has dtype {a.dtype}: a resident column is int32, int64, float32 or float64")
    a = np.ascontiguousarray(a)
    if valid is not None:
        v = np.asarray(valid)
        if v.dtype != np.bool_ and v.dtype != np.uint8:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"valid must be a bool or uint8 array, got {v.dtype}")
        if v.shape != a.shape:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"valid has {v.size} entries for {a.size} values")
        valid = np.ascontiguousarray(v).view(np.uint8) if v.dtype == np.bool_ else np.ascontiguousarray(v)
    return a, valid, _COLUMN_DTYPES[a.dtype]


class Column:
    """A scalar column resident on one GPU (pqv.h: pqv_column): one value per corpus row, optional validity bytes (0 = NULL).
    What predicates (pqv.col(name) >= 2 ...) read; attach it to a searcher with Searcher.attach_column(name, column)."""

    def __init__(self, handle, keepalive=None):
        self._h = handle
        self._keepalive = keepalive

    @classmethod
    def upload(cls, values, valid=None, device=0):
        a, v, dtype = scalar_arrays(values, valid)
        h = vp()
        _check(_ffi.lib().pqv_column_upload(device, dtype, vp(a.ctypes.data), v.ctypes.data_as(_ffi.u8p) if v is not None else None,
                                            a.size, C.byref(h)))
        return cls(h)

    @classmethod
    def from_device_ptr(cls, dtype, ptr, n_rows, valid_ptr=0, device=0, keepalive=None):
        """Borrow device arrays (dtype: PQV_COL_*; valid_ptr: optional u8 [n_rows]); keepalive keeps their owner alive."""
        h = vp()
        _check(_ffi.lib().pqv_column_from_device(device, int(dtype), vp(ptr or None), vp(valid_ptr or None), int(n_rows), C.byref(h)))
        return cls(h, keepalive)

    @property
    def rows(self):
        return int(_ffi.lib().pqv_column_rows(self._h)) if self._h else 0

    @property
    def dtype(self):
        """PQV_COL_I32 / I64 / F32 / F64"""
        return int(_ffi.lib().pqv_column_dtype(self._h)) if self._h else -1

    @property
    def device(self):
        return int(_ffi.lib().pqv_column_device(self._h)) if self._h else -1

    def close(self):
        if self._h:
            _ffi.lib().pqv_column_free(self._h)
            self._h = None
            self._keepalive = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowMask:
    """One allow bit per row of a searcher's corpus (pqv.h: pqv_row_mask): made by Searcher.row_mask / row_mask_from_rows /
    row_mask_device, passed as mask= to that searcher's topk / range_search / topk_device.  Immutable; close() releases it."""

    def __init__(self, handle, searcher):
        self._h = handle
        self._searcher = searcher

    @property
    def rows(self):
        return int(_ffi.lib().pqv_row_mask_rows(self._h)) if self._h else 0

    @property
    def count(self):
        """allowed rows (that belong to an inverted list)"""
        return int(_ffi.lib().pqv_row_mask_count(self._h)) if self._h else 0

    def to_bytes(self):
        """uint8 [corpus rows]: 1 where the row is allowed -- every corpus row, whether or not it belongs to a list."""
        if self._h is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "row mask must not be NULL")
        out = np.zeros(self.rows, dtype=np.uint8)
        _check(_ffi.lib().pqv_row_mask_to_bytes(self._h, out.ctypes.data_as(_ffi.u8p), out.size))
        return out

    def close(self):
        if self._h:
            _ffi.lib().pqv_row_mask_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RowKeys:
    """A key column laid out for one searcher (pqv.h: pqv_row_keys): made by Searcher.row_keys, passed as keys= with one
    query_keys entry per query to that searcher's topk / range_search / topk_device -- every query is filtered by ITS OWN
    `column == key`.  Immutable; close() releases it."""

    def __init__(self, handle, searcher):
        self._h = handle
        self._searcher = searcher

    @property
    def rows(self):
        return int(_ffi.lib().pqv_row_keys_rows(self._h)) if self._h else 0

    @property
    def dtype(self):
        """PQV_COL_I32 or PQV_COL_I64"""
        return int(_ffi.lib().pqv_row_keys_dtype(self._h)) if self._h else -1

    def close(self):
        if self._h:
            _ffi.lib().pqv_row_keys_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _keys_handle(keys, query_keys):
    if not isinstance(keys, RowKeys):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"keys must be a RowKeys, got {type(keys).__name__}")
    if keys._h is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "row keys must not be NULL")
    if query_keys is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "query keys must not be NULL")
    return keys._h


def _group_handle(keys):
    if not isinstance(keys, RowKeys):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"keys must be a RowKeys, got {type(keys).__name__}")
    if keys._h is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "row keys must not be NULL")
    return keys._h


def _query_keys(query_keys, nq):
    """A host call's query keys -> contiguous int64 [nq]; integers only, each within i64."""
    a = np.asarray(query_keys)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"query keys must be integers, got {a.dtype}")
    if a.dtype == np.uint64 and a.size and int(a.max()) > 0x7FFFFFFFFFFFFFFF:
        raise PqvError(_ffi.PQV_ERR_INVALID, "query keys must fit int64")
    a = np.ascontiguousarray(a.reshape(-1), dtype=np.int64)
    if a.size != nq:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{a.size} query keys for {nq} queries")
    return a


def key_sets_to_csr(query_key_sets, nq):
    """A host call's query key sets (a sequence of nq iterables of integers) -> (lims uint64 [nq + 1], vals int64): every set
    sorted with duplicates removed, as pqv.h: PQV_KEY_IN wants it.  ValueError beyond PQV_KEY_SET_MAX distinct values in a set."""
    sets = list(query_key_sets)
    if len(sets) != nq:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{len(sets)} query key sets for {nq} queries")
    parts = []
    lims = np.zeros(nq + 1, dtype=np.uint64)
    for i, one in enumerate(sets):
        a = np.asarray(one if isinstance(one, np.ndarray) else list(one))
        if a.size and not np.issubdtype(a.dtype, np.integer):
            raise PqvError(_ffi.PQV_ERR_INVALID, f"query keys must be integers, got {a.dtype}")
        if a.dtype == np.uint64 and a.size and int(a.max()) > 0x7FFFFFFFFFFFFFFF:
            raise PqvError(_ffi.PQV_ERR_INVALID, "query keys must fit int64")
        a = np.unique(a.reshape(-1).astype(np.int64))
        if a.size > _ffi.PQV_KEY_SET_MAX:
            raise ValueError(f"a query key set takes at most {_ffi.PQV_KEY_SET_MAX} values, query {i} has {a.size}")
        parts.append(a)
        lims[i + 1] = lims[i] + np.uint64(a.size)
    vals = np.ascontiguousarray(np.concatenate(parts) if parts else np.zeros(0, dtype=np.int64), dtype=np.int64)
    if vals.size == 0:
        vals = np.zeros(1, dtype=np.int64)      # (never read: a readable address for the descriptor)
    return lims, vals


def _key_filter(keys, query_keys, query_key_ranges, query_key_sets, nq, device=False):
    """The per-query filter of a call: None (no keys= argument), ("keyed", handle, int64 array or device pointer) for query_keys=, or
    ("filtered", handle, KeyFilter, the arrays it points at) for query_key_ranges= / query_key_sets=.  Exactly one of the three goes
    with keys=."""
    given = [n for n, v in (("query_keys", query_keys), ("query_key_ranges", query_key_ranges), ("query_key_sets", query_key_sets))
             if v is not None]
    if keys is None and not given:
        return None
    if len(given) > 1:
        raise PqvError(_ffi.PQV_ERR_INVALID, " and ".join(given) + " are mutually exclusive")
    if query_key_ranges is None and query_key_sets is None:
        kh = _keys_handle(keys, query_keys)
        return ("keyed", kh, query_keys if device else _query_keys(query_keys, nq))
    kh = _keys_handle(keys, True)
    if query_key_ranges is not None:
        try:
            lo, hi = query_key_ranges
        except (TypeError, ValueError):
            raise PqvError(_ffi.PQV_ERR_INVALID, "query_key_ranges must be a pair (lo, hi)") from None
        if device:
            return ("filtered", kh, _ffi.KeyFilter(_ffi.PQV_KEY_RANGE, 0, int(lo) or None, int(hi) or None), ())
        lo, hi = _query_keys(lo, nq), _query_keys(hi, nq)
        return ("filtered", kh, _ffi.KeyFilter(_ffi.PQV_KEY_RANGE, 0, lo.ctypes.data, hi.ctypes.data), (lo, hi))
    if device:
        try:
            d_lims, d_vals = query_key_sets
        except (TypeError, ValueError):
            raise PqvError(_ffi.PQV_ERR_INVALID, "query_key_sets of a device call must be a pair (ptr_lims, ptr_vals)") from None
        return ("filtered", kh, _ffi.KeyFilter(_ffi.PQV_KEY_IN, 0, int(d_lims) or None, int(d_vals) or None), ())
    lims, vals = key_sets_to_csr(query_key_sets, nq)
    return ("filtered", kh, _ffi.KeyFilter(_ffi.PQV_KEY_IN, 0, lims.ctypes.data, vals.ctypes.data), (lims, vals))


def _probe_depth(probe_depths, d2_ratio, max_nprobe, max_candidates, mask, kf, nq, device=False):
    """The pqv_probe_depth descriptor of a topk / topk_device call with probe_depths= or d2_ratio= (pqv.h: pqv_topk_depth), and
    what must stay alive behind it.  Exactly one of the two, max_nprobe with it, and neither filter nor max_candidates."""
    if probe_depths is not None and d2_ratio is not None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "probe_depths and d2_ratio are mutually exclusive")
    if max_nprobe is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "probe_depths / d2_ratio need max_nprobe")
    if max_candidates:
        raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
    if mask is not None or kf is not None:
        raise PqvError(_ffi.PQV_ERR_UNSUPPORTED, "probe_depths / d2_ratio do not combine with mask= or keys= (pqv.h: pqv_topk_depth)")
    if d2_ratio is not None:
        return _ffi.ProbeDepth(_ffi.PQV_DEPTH_RATIO, max_nprobe, float(d2_ratio), None), None
    if device:
        return _ffi.ProbeDepth(_ffi.PQV_DEPTH_GIVEN, max_nprobe, 0.0, int(probe_depths) or None), None
    arr = np.asarray(probe_depths)
    if arr.shape != (nq,) or arr.dtype.kind not in "iu" or (arr.size and (arr.min() < 0 or arr.max() > 0xFFFFFFFF)):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"probe_depths must be {nq} integers in [0, 2^32)")
    arr = np.ascontiguousarray(arr, dtype=np.uint32)
    return _ffi.ProbeDepth(_ffi.PQV_DEPTH_GIVEN, max_nprobe, 0.0, arr.ctypes.data), arr


def _expand_filter(kf, device=False):
    """An expanding call's (keys handle, KeyFilter pointer, what must stay alive) from _key_filter's answer: query_keys= travels as a
    PQV_KEY_EQ descriptor (pqv.h: pqv_topk_expand); no keys= gives (None, None, ())."""
    if kf is None:
        return None, None, ()
    if kf[0] == "filtered":
        return kf[1], C.byref(kf[2]), kf
    qk = kf[2]
    f = _ffi.KeyFilter(_ffi.PQV_KEY_EQ, 0, (int(qk) or None) if device else qk.ctypes.data, None)
    return kf[1], C.byref(f), (kf, f)


def _group_filter(filter_keys, query_keys, query_key_ranges, query_key_sets, nq, device=False):
    """A distinct / grouped call's per-query filter: None without any of the four keywords (the unfiltered symbols are called), else
    _expand_filter's triple.  filter_keys= goes with exactly one of the three query keywords."""
    given = [n for n, v in (("query_keys", query_keys), ("query_key_ranges", query_key_ranges), ("query_key_sets", query_key_sets))
             if v is not None]
    if filter_keys is None and not given:
        return None
    if filter_keys is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, given[0] + " needs filter_keys=")
    if not given:
        raise PqvError(_ffi.PQV_ERR_INVALID, "filter_keys= needs query_keys=, query_key_ranges= or query_key_sets=")
    return _expand_filter(_key_filter(filter_keys, query_keys, query_key_ranges, query_key_sets, nq, device=device), device=device)


class KeyPartition:
    """A posting list per key value over one searcher's rows (pqv.h: pqv_key_partition): made by Searcher.key_partition, passed to
    that searcher's topk_partition / topk_partition_device -- the exact top-k over a key's own rows, nothing probed.  Immutable;
    close() releases it."""

    def __init__(self, handle, searcher):
        self._h = handle
        self._searcher = searcher

    @property
    def rows(self):
        """indexed rows with a valid key"""
        return int(_ffi.lib().pqv_key_partition_rows(self._h)) if self._h else 0

    @property
    def n_keys(self):
        """distinct key values among them"""
        return int(_ffi.lib().pqv_key_partition_n_keys(self._h)) if self._h else 0

    @property
    def dtype(self):
        """PQV_COL_I32 or PQV_COL_I64"""
        return int(_ffi.lib().pqv_key_partition_dtype(self._h)) if self._h else -1

    def keys(self, n=None):
        """(values int64, counts uint64): the first min(n, n_keys) distinct key values ascending and their row counts."""
        if self._h is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "key partition must not be NULL")
        n = self.n_keys if n is None else min(int(n), self.n_keys)
        vals = np.zeros(n, dtype=np.int64)
        counts = np.zeros(n, dtype=np.uint64)
        _check(_ffi.lib().pqv_key_partition_keys(self._h, vals.ctypes.data_as(_ffi.i64p), counts.ctypes.data_as(u64p), n))
        return vals, counts

    def close(self):
        if self._h:
            _ffi.lib().pqv_key_partition_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _partition_filter(part, query_keys, query_key_ranges, query_key_sets, nq, device=False):
    """A partition call's (partition handle, KeyFilter, what must stay alive): exactly one of the three query keywords, read as
    _key_filter reads them (query_keys= travels as a PQV_KEY_EQ descriptor)."""
    if not isinstance(part, KeyPartition):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"part must be a KeyPartition, got {type(part).__name__}")
    if part._h is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "key partition must not be NULL")
    given = [n for n, v in (("query_keys", query_keys), ("query_key_ranges", query_key_ranges), ("query_key_sets", query_key_sets))
             if v is not None]
    if not given:
        raise PqvError(_ffi.PQV_ERR_INVALID, "query keys must not be NULL")
    if len(given) > 1:
        raise PqvError(_ffi.PQV_ERR_INVALID, " and ".join(given) + " are mutually exclusive")
    if query_keys is not None:
        if device:
            return part._h, _ffi.KeyFilter(_ffi.PQV_KEY_EQ, 0, int(query_keys) or None, None), ()
        qk = _query_keys(query_keys, nq)
        return part._h, _ffi.KeyFilter(_ffi.PQV_KEY_EQ, 0, qk.ctypes.data, None), (qk,)
    if query_key_ranges is not None:
        try:
            lo, hi = query_key_ranges
        except (TypeError, ValueError):
            raise PqvError(_ffi.PQV_ERR_INVALID, "query_key_ranges must be a pair (lo, hi)") from None
        if device:
            return part._h, _ffi.KeyFilter(_ffi.PQV_KEY_RANGE, 0, int(lo) or None, int(hi) or None), ()
        lo, hi = _query_keys(lo, nq), _query_keys(hi, nq)
        return part._h, _ffi.KeyFilter(_ffi.PQV_KEY_RANGE, 0, lo.ctypes.data, hi.ctypes.data), (lo, hi)
    if device:
        try:
            d_lims, d_vals = query_key_sets
        except (TypeError, ValueError):
            raise PqvError(_ffi.PQV_ERR_INVALID, "query_key_sets of a device call must be a pair (ptr_lims, ptr_vals)") from None
        return part._h, _ffi.KeyFilter(_ffi.PQV_KEY_IN, 0, int(d_lims) or None, int(d_vals) or None), ()
    lims, vals = key_sets_to_csr(query_key_sets, nq)
    return part._h, _ffi.KeyFilter(_ffi.PQV_KEY_IN, 0, lims.ctypes.data, vals.ctypes.data), (lims, vals)


def _row_ids_u32(ids, what="row ids"):
    """Row ids -> contiguous uint32: integers in [0, 2^32), checked as row_mask_from_rows checks its ids (a candidate list may name
    rows the corpus does not have: they are skipped by the call, not refused here)."""
    a = np.asarray(ids)
    if a.size and not np.issubdtype(a.dtype, np.integer):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} must be integers, got {a.dtype}")
    a = a.reshape(-1)
    if a.size and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} must be in [0, 2^32)")
    return np.ascontiguousarray(a, dtype=np.uint32)


def _candidate_lists(candidates, nq):
    """A candidate-list call's (lims uint64 [nq + 1], rows uint32): a TUPLE is a (lims, rows) pair passed on as given -- lims need not
    start at 0 --, any other sequence holds one integer array per query."""
    if candidates is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "candidates must not be None")
    if isinstance(candidates, tuple):
        if len(candidates) != 2:
            raise PqvError(_ffi.PQV_ERR_INVALID, "candidates given as a tuple must be a pair (lims, rows)")
        lims = np.asarray(candidates[0])
        if lims.ndim != 1 or lims.size != nq + 1:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"lims must have nq + 1 = {nq + 1} entries, got shape {lims.shape}")
        if not np.issubdtype(lims.dtype, np.integer) or (lims.size and int(lims.min()) < 0):
            raise PqvError(_ffi.PQV_ERR_INVALID, "lims must be non-negative integers")
        rows = _row_ids_u32(candidates[1], "candidate row ids")
        if int(lims.max()) > rows.size:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"lims reach {int(lims.max())}, the candidate rows hold {rows.size} ids")
        return np.ascontiguousarray(lims, dtype=np.uint64), rows
    try:
        per_query = [_row_ids_u32(c, "candidate row ids") for c in candidates]
    except TypeError:
        raise PqvError(_ffi.PQV_ERR_INVALID, "candidates must be a sequence of per-query integer arrays or a (lims, rows) tuple") from None
    if len(per_query) != nq:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"candidates has {len(per_query)} lists, the call has {nq} queries")
    lims = np.zeros(nq + 1, dtype=np.uint64)
    if nq:
        lims[1:] = np.cumsum([c.size for c in per_query], dtype=np.uint64)
    rows = np.concatenate(per_query) if per_query else np.zeros(0, dtype=np.uint32)
    return lims, np.ascontiguousarray(rows, dtype=np.uint32)


def _allow_array(allowed, n_rows, what="row mask"):
    """A caller's allow array -> contiguous uint8 [n_rows]: bool or uint8, one entry per row; anything else is refused."""
    if allowed is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} must not be None")
    a = np.asarray(allowed)
    if a.dtype != np.bool_ and a.dtype != np.uint8:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} must be a bool or uint8 array, got {a.dtype}")
    if a.ndim != 1:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"{what} must be one-dimensional, got {a.ndim} dimensions")
    if n_rows is not None and a.size != n_rows:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"row mask has {a.size} rows, the corpus has {n_rows}")
    return np.ascontiguousarray(a).view(np.uint8) if a.dtype == np.bool_ else np.ascontiguousarray(a)


def _take_range_buffers(nq, lims_p, rows_p, dist_p):
    """(lims, rows, dist) copied out of a range call's library buffers, which are released"""
    try:
        lims = np.ctypeslib.as_array(lims_p, shape=(nq + 1,)).copy()
        total = int(lims[-1])
        rows = (np.ctypeslib.as_array(rows_p, shape=(total,)).copy() if total else np.zeros(0, dtype=np.uint32))
        dist = (np.ctypeslib.as_array(dist_p, shape=(total,)).copy() if total else np.zeros(0, dtype=np.float32))
    finally:
        _ffi.lib().pqv_range_free(lims_p, rows_p, dist_p)
    return lims, rows, dist


def _mask_handle(searcher, mask):
    if not isinstance(mask, RowMask):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"mask must be a RowMask, got {type(mask).__name__}")
    if mask._h is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "row mask must not be NULL")
    return mask._h


class Searcher:
    """An index bound to a resident corpus on that corpus' GPU."""

    def __init__(self, index, corpus, flags=_ffi.PQV_LAYOUT_IVF_ORDERED):
        h = vp()
        _check(_ffi.lib().pqv_searcher_create(index._h, corpus._h, flags, C.byref(h)))
        self._h = h
        self._corpus = corpus
        self._columns = {}           # name -> Column (attach_column)
        self._owned_columns = []     # the attached columns that close() closes
        self.dim = index.dim
        self.n_clusters = index.n_clusters

    def probe(self, query, nprobe):
        q = _f32(query).reshape(-1)
        out = np.zeros(max(1, min(nprobe, self.n_clusters)), dtype=np.uint32)
        n = C.c_uint32(0)
        _check(_ffi.lib().pqv_probe(self._h, q.ctypes.data_as(f32p), q.size, nprobe,
                                    out.ctypes.data_as(u32p), C.byref(n)))
        return out[:n.value].copy()

    def candidate_rows(self, query, nprobe):
        q = _f32(query).reshape(-1)
        rows = u32p()
        n = C.c_uint64(0)
        _check(_ffi.lib().pqv_candidate_rows(self._h, q.ctypes.data_as(f32p), q.size, nprobe,
                                             C.byref(rows), C.byref(n)))
        try:
            return (np.ctypeslib.as_array(rows, shape=(n.value,)).copy() if n.value
                    else np.zeros(0, dtype=np.uint32))
        finally:
            _ffi.lib().pqv_rows_free(rows)

    @property
    def columns(self):
        """{name: Column}: the scalar columns attached to this searcher (what predicates' names resolve against)."""
        return self._columns

    def attach_column(self, name, column, own=False):
        """Make a resident scalar column known to predicates as `name`: a Column, or a numpy / pyarrow array that is uploaded to
        the searcher's device.  One value per corpus row.  Returns the Column.  close() closes the columns the searcher uploaded
        itself and those attached with own=True; any other Column stays its caller's (it may serve several searchers)."""
        if not isinstance(name, str) or not name:
            raise PqvError(_ffi.PQV_ERR_INVALID, "attach_column needs a column name")
        if not isinstance(column, Column):
            a, v, _ = scalar_arrays(column, name=name)
            if a.size != self._corpus.rows:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"column has {a.size} rows, the corpus has {self._corpus.rows}")
            column = Column.upload(a, v, device=self._corpus.device)
            own = True
        elif column._h is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "column must not be NULL")
        self._columns[name] = column
        if own:
            self._owned_columns.append(column)
        return column

    def row_mask_predicate(self, pred, stream=0):
        """RowMask of a predicate over the attached columns (pqv.h: pqv_row_mask_from_predicates): evaluated on the device; the
        only host traffic is the leaf table in and the allowed count out.  Complete on return."""
        cols = self.columns
        for name in pred.columns():
            if name not in cols:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"no column named {name!r} is attached to this searcher")
        comp = predicate.compile(pred, {name: c.dtype for name, c in cols.items()})
        n = len(comp.leaves)
        col_h = (vp * n)(*[cols[x]._h if isinstance(x, str) else None for x in comp.leaves])
        mask_h = (vp * n)(*[None if isinstance(x, str) else _mask_handle(self, x) for x in comp.leaves])
        prog = np.frombuffer(comp.program, dtype=np.uint8)
        h = vp()
        _check(_ffi.lib().pqv_row_mask_from_predicates(self._h, n, col_h, mask_h, comp.ops.ctypes.data_as(u32p),
                                                       comp.operands.ctypes.data_as(u64p), prog.ctypes.data_as(_ffi.u8p), prog.size,
                                                       vp(stream or None), C.byref(h)))
        return RowMask(h, self)

    def row_mask(self, allowed):
        """RowMask from a bool / uint8 array [corpus rows] (nonzero = allowed), or from a predicate over the attached columns
        (pqv.col(name) >= 2 ...: row_mask_predicate)."""
        if isinstance(allowed, predicate.Predicate):
            return self.row_mask_predicate(allowed)
        a = _allow_array(allowed, self._corpus.rows)
        h = vp()
        _check(_ffi.lib().pqv_row_mask_create(self._h, a.ctypes.data_as(_ffi.u8p), a.size, C.byref(h)))
        return RowMask(h, self)

    def row_mask_from_rows(self, row_ids, allow=True):
        """RowMask that allows exactly `row_ids` -- or, with allow=False, every row BUT these (deletions)."""
        n = self._corpus.rows
        ids = np.asarray(row_ids)
        if ids.size and not np.issubdtype(ids.dtype, np.integer):
            raise PqvError(_ffi.PQV_ERR_INVALID, f"row ids must be integers, got {ids.dtype}")
        ids = ids.reshape(-1).astype(np.int64)
        if ids.size and (ids.min() < 0 or ids.max() >= n):
            raise PqvError(_ffi.PQV_ERR_INVALID, f"row id out of range for a corpus of {n} rows")
        a = np.zeros(n, dtype=np.uint8) if allow else np.ones(n, dtype=np.uint8)
        a[ids] = 1 if allow else 0
        return self.row_mask(a)

    def row_mask_device(self, ptr, n_rows, stream=0):
        """RowMask from device bytes u8 [n_rows] (e.g. a torch.bool tensor's data_ptr()); complete on return."""
        h = vp()
        _check(_ffi.lib().pqv_row_mask_from_device(self._h, vp(ptr or None), int(n_rows), vp(stream or None), C.byref(h)))
        return RowMask(h, self)

    def row_keys(self, column, stream=0):
        """RowKeys of an integer column (a Column, or the name of an attached one): pqv.h: pqv_row_keys_create.  The column is
        copied, so it may be closed afterwards.  Complete on return."""
        if isinstance(column, str):
            if column not in self._columns:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"no column named {column!r} is attached to this searcher")
            column = self._columns[column]
        if not isinstance(column, Column) or column._h is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "column must not be NULL")
        h = vp()
        _check(_ffi.lib().pqv_row_keys_create(self._h, column._h, vp(stream or None), C.byref(h)))
        return RowKeys(h, self)

    def key_partition(self, column, stream=0):
        """KeyPartition of an integer column (a Column, or the name of an attached one): pqv.h: pqv_key_partition_create.  Built on
        the device; the column may be closed afterwards.  Complete on return."""
        if isinstance(column, str):
            if column not in self._columns:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"no column named {column!r} is attached to this searcher")
            column = self._columns[column]
        if not isinstance(column, Column) or column._h is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "column must not be NULL")
        h = vp()
        _check(_ffi.lib().pqv_key_partition_create(self._h, column._h, vp(stream or None), C.byref(h)))
        return KeyPartition(h, self)

    def topk_partition(self, queries, k, part, query_keys=None, query_key_ranges=None, query_key_sets=None, mask=None,
                       metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """Exact top-k over the rows of `part` (a KeyPartition of this searcher) whose key passes the query's filter -- exactly one
        of query_keys (int [nq]), query_key_ranges=(lo, hi) or query_key_sets, read as topk reads them -- within mask if one is
        given; nothing is probed (pqv.h: pqv_topk_partition).  Returns (row_idx [nq,k] u32, dist [nq,k] f32, n_found [nq],
        n_candidates [nq])."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        ph, f, _alive = _partition_filter(part, query_keys, query_key_ranges, query_key_sets, nq)
        rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        _check(_ffi.lib().pqv_topk_partition(self._h, ph, C.byref(f), _mask_handle(self, mask) if mask is not None else None,
                                             q.ctypes.data_as(f32p), nq, qlen, k, metric, 1 if sqrt_out else 0,
                                             rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p),
                                             nc.ctypes.data_as(u64p)))
        return rows, dist, nf, nc

    def topk_partition_device(self, d_queries, nq, k, part, d_row_idx, d_dist, d_n_found=0, d_n_candidates=0, query_keys=None,
                              query_key_ranges=None, query_key_sets=None, mask=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0):
        """Device-pointer form of topk_partition, shaped like topk_device: asynchronous on `stream`; the query keywords take device
        pointers (int64 [nq]; (ptr_lo, ptr_hi); (ptr_lims, ptr_vals)) read on `stream` inside the enqueued work (pqv.h:
        pqv_topk_partition_device)."""
        ph, f, _alive = _partition_filter(part, query_keys, query_key_ranges, query_key_sets, nq, device=True)
        _check(_ffi.lib().pqv_topk_partition_device(self._h, ph, C.byref(f), _mask_handle(self, mask) if mask is not None else None,
                                                    vp(d_queries), nq, k, metric, 1 if sqrt_out else 0, vp(d_row_idx), vp(d_dist),
                                                    vp(d_n_found or None), vp(d_n_candidates or None), vp(stream or None)))

    def topk_rows(self, queries, k, candidates, mask=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """Exact top-k among the rows the caller names per query -- `candidates`: a list of per-query integer arrays, or a
        (lims, rows) TUPLE (lims int [nq + 1], need not start at 0; rows the ids, query q's are rows[lims[q]:lims[q + 1]]) -- in any
        order, duplicates allowed, within mask if one is given; nothing is probed (pqv.h: pqv_topk_rows).  Returns (row_idx [nq,k]
        u32, dist [nq,k] f32, n_found [nq], n_candidates [nq])."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        lims, cand = _candidate_lists(candidates, nq)
        rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        _check(_ffi.lib().pqv_topk_rows(self._h, lims.ctypes.data_as(u64p), cand.ctypes.data_as(u32p),
                                        _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq, qlen, k, metric,
                                        1 if sqrt_out else 0, rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p),
                                        nc.ctypes.data_as(u64p)))
        return rows, dist, nf, nc

    def score_rows(self, queries, candidates, mask=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """The exact distance of every candidate (`candidates` as topk_rows takes them) to its query, +inf for a row that is not
        indexed or that mask excludes (pqv.h: pqv_score_rows).  Returns (lims u64 [nq + 1] rebased to start at 0, dist f32
        [lims[nq]]): query q's distances are dist[lims[q]:lims[q + 1]], in the order its candidates were given."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        lims, cand = _candidate_lists(candidates, nq)
        total = int(lims[nq] - lims[0]) if lims[nq] >= lims[0] else 0
        dist = np.full(max(total, 1), np.inf, dtype=np.float32)
        _check(_ffi.lib().pqv_score_rows(self._h, lims.ctypes.data_as(u64p), cand.ctypes.data_as(u32p),
                                         _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq, qlen, metric,
                                         1 if sqrt_out else 0, dist.ctypes.data_as(f32p)))
        return lims - lims[0], dist[:total]

    def topk_rows_device(self, d_queries, nq, k, d_lims, d_cand_rows, d_row_idx, d_dist, d_n_found=0, d_n_candidates=0, mask=None,
                         metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0):
        """Device-pointer form of topk_rows, shaped like topk_device: asynchronous on `stream`; d_lims (u64 [nq + 1]) and d_cand_rows
        (u32) are device pointers read on `stream` inside the enqueued work (pqv.h: pqv_topk_rows_device).  The first candidate-list
        call on a searcher builds its row map and waits for it."""
        _check(_ffi.lib().pqv_topk_rows_device(self._h, vp(d_lims or None), vp(d_cand_rows or None),
                                               _mask_handle(self, mask) if mask is not None else None, vp(d_queries or None), nq, k, metric,
                                               1 if sqrt_out else 0, vp(d_row_idx or None), vp(d_dist or None), vp(d_n_found or None),
                                               vp(d_n_candidates or None), vp(stream or None)))

    def score_rows_device(self, d_queries, nq, d_lims, d_cand_rows, d_dist, mask=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0):
        """Device-pointer form of score_rows: d_dist f32 [lims[nq] - lims[0]], candidate i's distance at i - lims[0]; asynchronous on
        `stream` (pqv.h: pqv_score_rows_device)."""
        _check(_ffi.lib().pqv_score_rows_device(self._h, vp(d_lims or None), vp(d_cand_rows or None),
                                                _mask_handle(self, mask) if mask is not None else None, vp(d_queries or None), nq, metric,
                                                1 if sqrt_out else 0, vp(d_dist or None), vp(stream or None)))

    def topk_mmr(self, queries, k, fetch_k, nprobe, lambda_=0.5, mask=None, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """MMR top-k: the fetch_k nearest rows of the probed lists (within mask if one is given), then k of them picked greedily by
        (lambda_ * distance) - ((1 - lambda_) * distance to the nearest row picked so far), smallest first -- lambda_ = 1 is the plain
        top-k, smaller values trade relevance for diversity (pqv.h: pqv_topk_mmr).  Returns (row_idx [nq,k] u32, dist [nq,k] f32,
        score [nq,k] f32, n_found [nq], n_candidates [nq]) in PICK order."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        score = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        _check(_ffi.lib().pqv_topk_mmr(self._h, _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq, qlen, k,
                                       fetch_k, float(lambda_), nprobe, max_candidates, metric, 1 if sqrt_out else 0, rows.ctypes.data_as(u32p),
                                       dist.ctypes.data_as(f32p), score.ctypes.data_as(f32p), nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p)))
        return rows, dist, score, nf, nc

    def mmr_select(self, rows, dist, k, lambda_=0.5, n_found=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """The MMR selection alone over candidates the caller has: rows u32 [nq, n] and dist f32 [nq, n], the outputs of ANY top-k
        call of this searcher with the same metric and sqrt_out, and optionally its n_found [nq] (pqv.h: pqv_mmr_select).  Returns
        (row_idx [nq,k] u32, dist [nq,k] f32, score [nq,k] f32, n_found [nq]) in PICK order."""
        cand = np.ascontiguousarray(rows, dtype=np.uint32)
        rel = _f32(dist)
        if cand.ndim == 1:
            cand = cand.reshape(1, -1)
        if rel.ndim == 1:
            rel = rel.reshape(1, -1)
        if cand.ndim != 2 or cand.shape != rel.shape:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"mmr_select needs rows and dist of one [nq, n] shape, got {cand.shape} and {rel.shape}")
        nq, n = cand.shape
        nf_in = None
        if n_found is not None:
            nf_in = np.ascontiguousarray(n_found, dtype=np.uint32).reshape(-1)
            if nf_in.shape[0] != nq:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"mmr_select needs n_found of length {nq}, got {nf_in.shape[0]}")
        out_rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        out_dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        score = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        nf = np.zeros(nq, dtype=np.uint32)
        _check(_ffi.lib().pqv_mmr_select(self._h, cand.ctypes.data_as(u32p), rel.ctypes.data_as(f32p),
                                         nf_in.ctypes.data_as(u32p) if nf_in is not None else None, nq, n, k, float(lambda_), metric,
                                         1 if sqrt_out else 0, out_rows.ctypes.data_as(u32p), out_dist.ctypes.data_as(f32p),
                                         score.ctypes.data_as(f32p), nf.ctypes.data_as(u32p)))
        return out_rows, out_dist, score, nf

    def topk_mmr_device(self, d_queries, nq, k, fetch_k, nprobe, d_row_idx, d_dist, d_score=0, d_n_found=0, d_n_candidates=0, lambda_=0.5,
                        mask=None, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0):
        """Device-pointer form of topk_mmr, shaped like topk_device: asynchronous on `stream` (pqv.h: pqv_topk_mmr_device).  The first
        call on a searcher that needs its row map builds it and waits for it."""
        _check(_ffi.lib().pqv_topk_mmr_device(self._h, _mask_handle(self, mask) if mask is not None else None, vp(d_queries or None), nq, k,
                                              fetch_k, float(lambda_), nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                              vp(d_row_idx or None), vp(d_dist or None), vp(d_score or None), vp(d_n_found or None),
                                              vp(d_n_candidates or None), vp(stream or None)))

    def mmr_select_device(self, d_cand_rows, d_cand_dist, nq, n, k, d_row_idx, d_dist, d_score=0, d_n_found=0, d_n_found_in=0, lambda_=0.5,
                          metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0):
        """Device-pointer form of mmr_select: d_cand_rows u32 / d_cand_dist f32 [nq, n] and the optional d_n_found_in u32 [nq] are read
        on `stream` inside the enqueued work (pqv.h: pqv_mmr_select_device)."""
        _check(_ffi.lib().pqv_mmr_select_device(self._h, vp(d_cand_rows or None), vp(d_cand_dist or None), vp(d_n_found_in or None), nq, n, k,
                                                float(lambda_), metric, 1 if sqrt_out else 0, vp(d_row_idx or None), vp(d_dist or None),
                                                vp(d_score or None), vp(d_n_found or None), vp(stream or None)))

    def topk_partition_grouped(self, queries, k, group_size, part, keys, query_keys=None, query_key_ranges=None, query_key_sets=None,
                               mask=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """Exact grouped top-k over the rows of `part` whose key passes the query's filter (the keywords of topk_partition): up
        to group_size rows of each of the k nearest groups of `keys` -- a RowKeys of this searcher, or the name of an attached
        column -- within mask if one is given; nothing is probed (pqv.h: pqv_topk_partition_grouped).  Returns (row_idx
        [nq,k,group_size] u32, dist [nq,k,group_size] f32, group_keys [nq,k] i64, group_rows [nq,k] u32, n_found [nq],
        n_candidates [nq]), laid out and padded as topk_grouped's."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        ph, f, _alive = _partition_filter(part, query_keys, query_key_ranges, query_key_sets, nq)
        shape = (nq, max(k, 1), max(group_size, 1))
        rows = np.full(shape, 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full(shape, np.inf, dtype=np.float32)
        grp = np.zeros(shape[:2], dtype=np.int64)
        grows = np.zeros(shape[:2], dtype=np.uint32)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        owned = isinstance(keys, str)
        if owned:
            keys = self.row_keys(keys)
        try:
            kh = _group_handle(keys)
            _check(_ffi.lib().pqv_topk_partition_grouped(self._h, ph, C.byref(f), kh,
                                                         _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                         qlen, k, group_size, metric, 1 if sqrt_out else 0, rows.ctypes.data_as(u32p),
                                                         dist.ctypes.data_as(f32p), grp.ctypes.data_as(_ffi.i64p), grows.ctypes.data_as(u32p),
                                                         nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p)))
        finally:
            if owned:
                keys.close()
        return rows, dist, grp, grows, nf, nc

    def topk_partition_distinct(self, queries, k, part, keys, query_keys=None, query_key_ranges=None, query_key_sets=None, mask=None,
                                metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """Exact distinct top-k over a partition: topk_partition_grouped with group_size = 1.  Returns (row_idx [nq,k] u32, dist
        [nq,k] f32, group_keys [nq,k] i64, n_found [nq], n_candidates [nq])."""
        rows, dist, grp, _grows, nf, nc = self.topk_partition_grouped(queries, k, 1, part, keys, query_keys=query_keys,
                                                                      query_key_ranges=query_key_ranges, query_key_sets=query_key_sets,
                                                                      mask=mask, metric=metric, sqrt_out=sqrt_out)
        return rows.reshape(rows.shape[:2]), dist.reshape(dist.shape[:2]), grp, nf, nc

    def topk_partition_grouped_device(self, d_queries, nq, k, group_size, part, keys, d_row_idx, d_dist, d_group_key=0, d_group_rows=0,
                                      d_n_found=0, d_n_candidates=0, query_keys=None, query_key_ranges=None, query_key_sets=None,
                                      mask=None, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0):
        """Device-pointer form of topk_partition_grouped, shaped like topk_partition_device plus the two group outputs: d_row_idx
        u32 / d_dist f32 [nq, k, group_size], d_group_key i64 / d_group_rows u32 [nq, k], d_n_found u32 / d_n_candidates u64 [nq];
        the last four are optional.  Asynchronous on `stream`; the query keywords take device pointers read on `stream` inside
        the enqueued work.  `keys` (a RowKeys), `part` and `mask` must stay alive until the work has completed (pqv.h:
        pqv_topk_partition_grouped_device)."""
        ph, f, _alive = _partition_filter(part, query_keys, query_key_ranges, query_key_sets, nq, device=True)
        kh = _group_handle(keys)
        _check(_ffi.lib().pqv_topk_partition_grouped_device(self._h, ph, C.byref(f), kh,
                                                            _mask_handle(self, mask) if mask is not None else None, vp(d_queries), nq, k,
                                                            group_size, metric, 1 if sqrt_out else 0, vp(d_row_idx), vp(d_dist),
                                                            vp(d_group_key or None), vp(d_group_rows or None), vp(d_n_found or None),
                                                            vp(d_n_candidates or None), vp(stream or None)))

    def topk(self, queries, k, nprobe, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, mask=None, keys=None,
             query_keys=None, query_key_ranges=None, query_key_sets=None, max_nprobe=None, probe_depths=None, d2_ratio=None):
        """Batched topk(); returns (row_idx [nq,k] u32, dist [nq,k] f32, n_found [nq], n_candidates [nq]).
        probe_depths (int [nq]) or d2_ratio (float >= 1), with max_nprobe and no filter: per-query probe depths -- query q walks
        min(max(r, nprobe), max_nprobe) lists, r its given depth or the lists whose centroid is within d2_ratio (squared scale) of
        the nearest one, and gets what the plain call returns at that nprobe; a fifth array nprobe_used [nq] u32 comes back
        (pqv.h: pqv_topk_depth).
        max_nprobe (with mask= or keys=; not with max_candidates): keep probing until k rows pass the filter -- query q probes the
        fewest lists, at least nprobe and at most max_nprobe, whose passing rows number k, and gets what the call without
        max_nprobe returns for that many lists; a fifth array nprobe_used [nq] u32 comes back (pqv.h: pqv_topk_expand).
        mask (a RowMask of this searcher): only allowed rows are considered (pqv.h: pqv_topk_masked).
        keys (a RowKeys of this searcher) with query_keys (int [nq]): query q considers only the rows whose key equals
        query_keys[q], within mask if one is given too (pqv.h: pqv_topk_keyed).  Instead of query_keys:
        query_key_ranges=(lo, hi) (int [nq] each): lo[q] <= key <= hi[q], both inclusive; or query_key_sets (nq iterables of
        integers, at most PQV_KEY_SET_MAX distinct values each; sorted and de-duplicated here): key in the query's set
        (pqv.h: pqv_topk_filtered)."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        kf = _key_filter(keys, query_keys, query_key_ranges, query_key_sets, nq)
        if probe_depths is not None or d2_ratio is not None:
            d, _alive = _probe_depth(probe_depths, d2_ratio, max_nprobe, max_candidates, mask, kf, nq)
            used = np.zeros(nq, dtype=np.uint32)
            _check(_ffi.lib().pqv_topk_depth(self._h, C.byref(d), q.ctypes.data_as(f32p), nq, qlen, k, nprobe, metric,
                                             1 if sqrt_out else 0, rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p),
                                             nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p), used.ctypes.data_as(u32p)))
            return rows, dist, nf, nc, used
        if max_nprobe is not None:
            if max_candidates:
                raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
            used = np.zeros(nq, dtype=np.uint32)
            kh, fp, _alive = _expand_filter(kf)
            _check(_ffi.lib().pqv_topk_expand(self._h, kh, fp, _mask_handle(self, mask) if mask is not None else None,
                                              q.ctypes.data_as(f32p), nq, qlen, k, nprobe, max_nprobe, metric, 1 if sqrt_out else 0,
                                              rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p),
                                              nc.ctypes.data_as(u64p), used.ctypes.data_as(u32p)))
            return rows, dist, nf, nc, used
        if kf is not None and kf[0] == "filtered":
            _check(_ffi.lib().pqv_topk_filtered(self._h, kf[1], C.byref(kf[2]), _mask_handle(self, mask) if mask is not None else None,
                                                q.ctypes.data_as(f32p), nq, qlen, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p),
                                                nc.ctypes.data_as(u64p)))
            return rows, dist, nf, nc
        if kf is not None:
            kh, qk = kf[1], kf[2]
            _check(_ffi.lib().pqv_topk_keyed(self._h, kh, qk.ctypes.data_as(_ffi.i64p), _mask_handle(self, mask) if mask is not None else None,
                                             q.ctypes.data_as(f32p), nq, qlen, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                             rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p),
                                             nc.ctypes.data_as(u64p)))
            return rows, dist, nf, nc
        if mask is not None:
            _check(_ffi.lib().pqv_topk_masked(self._h, _mask_handle(self, mask), q.ctypes.data_as(f32p), nq, qlen, k, nprobe,
                                              max_candidates, metric, 1 if sqrt_out else 0, rows.ctypes.data_as(u32p),
                                              dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p)))
            return rows, dist, nf, nc
        _check(_ffi.lib().pqv_topk(self._h, q.ctypes.data_as(f32p), nq, qlen, k, nprobe, max_candidates,
                                   metric, 1 if sqrt_out else 0, rows.ctypes.data_as(u32p),
                                   dist.ctypes.data_as(f32p), nf.ctypes.data_as(u32p),
                                   nc.ctypes.data_as(u64p)))
        return rows, dist, nf, nc

    def topk_distinct(self, queries, k, nprobe, keys, mask=None, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True,
                      filter_keys=None, query_keys=None, query_key_ranges=None, query_key_sets=None, max_nprobe=None):
        """Distinct top-k (pqv.h: pqv_topk_distinct): per query the nearest row of each of the k nearest groups, a group being the
        considered rows of one value of `keys` (a RowKeys of this searcher; NULL-key rows belong to no group), under `mask` if one
        is given.  Returns (row_idx [nq,k] u32, dist [nq,k] f32, group_keys [nq,k] i64, n_found [nq], n_candidates [nq]), ascending
        by (d2, candidate position); entries past n_found are 0xFFFFFFFF, +inf and 0.
        filter_keys (a RowKeys of this searcher; it may be `keys`) with one of query_keys / query_key_ranges / query_key_sets, as
        topk takes them: query q considers only the rows whose filter key passes ITS test -- the filter applies before a group's
        representative is chosen (pqv.h: pqv_topk_distinct_filtered).
        max_nprobe (not with max_candidates): keep probing until k GROUPS are found -- query q probes the fewest lists, at least
        nprobe and at most max_nprobe, that hold k distinct group values among its considered rows, and gets what the call without
        max_nprobe returns for that many lists; a sixth array nprobe_used [nq] u32 comes back (pqv.h: pqv_topk_distinct_expand)."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        rows = np.full((nq, max(k, 1)), 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full((nq, max(k, 1)), np.inf, dtype=np.float32)
        grp = np.zeros((nq, max(k, 1)), dtype=np.int64)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        gf = _group_filter(filter_keys, query_keys, query_key_ranges, query_key_sets, nq)
        if max_nprobe is not None:
            if max_candidates:
                raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
            used = np.zeros(nq, dtype=np.uint32)
            fk, fp = (gf[0], gf[1]) if gf is not None else (None, None)
            _check(_ffi.lib().pqv_topk_distinct_expand(self._h, _group_handle(keys), fk, fp,
                                                       _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                       qlen, k, nprobe, max_nprobe, metric, 1 if sqrt_out else 0,
                                                       rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), grp.ctypes.data_as(_ffi.i64p),
                                                       nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p), used.ctypes.data_as(u32p)))
            return rows, dist, grp, nf, nc, used
        if gf is not None:
            _check(_ffi.lib().pqv_topk_distinct_filtered(self._h, _group_handle(keys), gf[0], gf[1],
                                                         _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                         qlen, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                         rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), grp.ctypes.data_as(_ffi.i64p),
                                                         nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p)))
            return rows, dist, grp, nf, nc
        _check(_ffi.lib().pqv_topk_distinct(self._h, _group_handle(keys), _mask_handle(self, mask) if mask is not None else None,
                                            q.ctypes.data_as(f32p), nq, qlen, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                            rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), grp.ctypes.data_as(_ffi.i64p),
                                            nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p)))
        return rows, dist, grp, nf, nc

    def topk_distinct_device(self, d_queries, nq, k, nprobe, keys, d_row_idx, d_dist, d_group_key=0, d_n_found=0, d_n_candidates=0,
                             mask=None, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0, filter_keys=None,
                             query_keys=None, query_key_ranges=None, query_key_sets=None, max_nprobe=0, d_nprobe_used=0):
        """Device-pointer form of topk_distinct (pqv.h: pqv_topk_distinct_device), asynchronous on `stream` as topk_device is:
        d_row_idx u32 / d_dist f32 / d_group_key i64 [nq, k], d_n_found u32 / d_n_candidates u64 [nq]; the last three are optional.
        keys and mask must stay alive until the enqueued work has completed.
        filter_keys with query_keys / query_key_ranges / query_key_sets as DEVICE pointers, as topk_device takes them, read on
        `stream` inside the enqueued work (pqv.h: pqv_topk_distinct_filtered_device).
        max_nprobe (> 0; not with max_candidates): the expanding call, as topk_distinct's; d_nprobe_used (u32 [nq], optional) takes
        the lists each query probed (pqv.h: pqv_topk_distinct_expand_device)."""
        gf = _group_filter(filter_keys, query_keys, query_key_ranges, query_key_sets, nq, device=True)
        if max_nprobe:
            if max_candidates:
                raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
            fk, fp = (gf[0], gf[1]) if gf is not None else (None, None)
            _check(_ffi.lib().pqv_topk_distinct_expand_device(self._h, _group_handle(keys), fk, fp,
                                                              _mask_handle(self, mask) if mask is not None else None, vp(d_queries), nq, k,
                                                              nprobe, max_nprobe, metric, 1 if sqrt_out else 0, vp(d_row_idx), vp(d_dist),
                                                              vp(d_group_key or None), vp(d_n_found or None), vp(d_n_candidates or None),
                                                              vp(d_nprobe_used or None), vp(stream or None)))
            return
        if gf is not None:
            _check(_ffi.lib().pqv_topk_distinct_filtered_device(self._h, _group_handle(keys), gf[0], gf[1],
                                                                _mask_handle(self, mask) if mask is not None else None, vp(d_queries), nq, k,
                                                                nprobe, max_candidates, metric, 1 if sqrt_out else 0, vp(d_row_idx),
                                                                vp(d_dist), vp(d_group_key or None), vp(d_n_found or None),
                                                                vp(d_n_candidates or None), vp(stream or None)))
            return
        _check(_ffi.lib().pqv_topk_distinct_device(self._h, _group_handle(keys), _mask_handle(self, mask) if mask is not None else None,
                                                   vp(d_queries), nq, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                   vp(d_row_idx), vp(d_dist), vp(d_group_key or None), vp(d_n_found or None),
                                                   vp(d_n_candidates or None), vp(stream or None)))

    def topk_grouped(self, queries, k, group_size, nprobe, keys, mask=None, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True,
                     filter_keys=None, query_keys=None, query_key_ranges=None, query_key_sets=None, max_nprobe=None):
        """Grouped top-k (pqv.h: pqv_topk_grouped): per query up to group_size rows of each of the k nearest groups of `keys` (as
        topk_distinct defines groups), under `mask` if one is given.  Returns (row_idx [nq,k,group_size] u32, dist [nq,k,group_size]
        f32, group_keys [nq,k] i64, group_rows [nq,k] u32, n_found [nq], n_candidates [nq]): groups ascending by their nearest row,
        a group's rows ascending by (d2, candidate position); empty row slots are 0xFFFFFFFF / +inf, empty groups key 0, count 0.
        filter_keys with query_keys / query_key_ranges / query_key_sets: a per-query filter, as topk_distinct takes it (pqv.h:
        pqv_topk_grouped_filtered).
        max_nprobe (not with max_candidates): keep probing until k groups are found, as topk_distinct takes it; a seventh array
        nprobe_used [nq] u32 comes back (pqv.h: pqv_topk_grouped_expand)."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        shape = (nq, max(k, 1), max(group_size, 1))
        rows = np.full(shape, 0xFFFFFFFF, dtype=np.uint32)
        dist = np.full(shape, np.inf, dtype=np.float32)
        grp = np.zeros(shape[:2], dtype=np.int64)
        grows = np.zeros(shape[:2], dtype=np.uint32)
        nf = np.zeros(nq, dtype=np.uint32)
        nc = np.zeros(nq, dtype=np.uint64)
        gf = _group_filter(filter_keys, query_keys, query_key_ranges, query_key_sets, nq)
        if max_nprobe is not None:
            if max_candidates:
                raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
            used = np.zeros(nq, dtype=np.uint32)
            fk, fp = (gf[0], gf[1]) if gf is not None else (None, None)
            _check(_ffi.lib().pqv_topk_grouped_expand(self._h, _group_handle(keys), fk, fp,
                                                      _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                      qlen, k, group_size, nprobe, max_nprobe, metric, 1 if sqrt_out else 0,
                                                      rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), grp.ctypes.data_as(_ffi.i64p),
                                                      grows.ctypes.data_as(u32p), nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p),
                                                      used.ctypes.data_as(u32p)))
            return rows, dist, grp, grows, nf, nc, used
        if gf is not None:
            _check(_ffi.lib().pqv_topk_grouped_filtered(self._h, _group_handle(keys), gf[0], gf[1],
                                                        _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                        qlen, k, group_size, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                        rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p), grp.ctypes.data_as(_ffi.i64p),
                                                        grows.ctypes.data_as(u32p), nf.ctypes.data_as(u32p), nc.ctypes.data_as(u64p)))
            return rows, dist, grp, grows, nf, nc
        _check(_ffi.lib().pqv_topk_grouped(self._h, _group_handle(keys), _mask_handle(self, mask) if mask is not None else None,
                                           q.ctypes.data_as(f32p), nq, qlen, k, group_size, nprobe, max_candidates, metric,
                                           1 if sqrt_out else 0, rows.ctypes.data_as(u32p), dist.ctypes.data_as(f32p),
                                           grp.ctypes.data_as(_ffi.i64p), grows.ctypes.data_as(u32p), nf.ctypes.data_as(u32p),
                                           nc.ctypes.data_as(u64p)))
        return rows, dist, grp, grows, nf, nc

    def topk_grouped_device(self, d_queries, nq, k, group_size, nprobe, keys, d_row_idx, d_dist, d_group_key=0, d_group_rows=0, d_n_found=0,
                            d_n_candidates=0, mask=None, max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0,
                            filter_keys=None, query_keys=None, query_key_ranges=None, query_key_sets=None, max_nprobe=0, d_nprobe_used=0):
        """Device-pointer form of topk_grouped (pqv.h: pqv_topk_grouped_device), asynchronous on `stream` as topk_device is:
        d_row_idx u32 / d_dist f32 [nq, k, group_size], d_group_key i64 / d_group_rows u32 [nq, k], d_n_found u32 / d_n_candidates u64
        [nq]; the last four are optional.  Serves k * group_size <= 1024.  keys and mask must stay alive until the work has completed.
        filter_keys with device-pointer query_keys / query_key_ranges / query_key_sets: as topk_distinct_device (pqv.h:
        pqv_topk_grouped_filtered_device).
        max_nprobe (> 0; not with max_candidates) and d_nprobe_used: the expanding call, as topk_distinct_device's (pqv.h:
        pqv_topk_grouped_expand_device)."""
        gf = _group_filter(filter_keys, query_keys, query_key_ranges, query_key_sets, nq, device=True)
        if max_nprobe:
            if max_candidates:
                raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
            fk, fp = (gf[0], gf[1]) if gf is not None else (None, None)
            _check(_ffi.lib().pqv_topk_grouped_expand_device(self._h, _group_handle(keys), fk, fp,
                                                             _mask_handle(self, mask) if mask is not None else None, vp(d_queries), nq, k,
                                                             group_size, nprobe, max_nprobe, metric, 1 if sqrt_out else 0, vp(d_row_idx),
                                                             vp(d_dist), vp(d_group_key or None), vp(d_group_rows or None),
                                                             vp(d_n_found or None), vp(d_n_candidates or None), vp(d_nprobe_used or None),
                                                             vp(stream or None)))
            return
        if gf is not None:
            _check(_ffi.lib().pqv_topk_grouped_filtered_device(self._h, _group_handle(keys), gf[0], gf[1],
                                                               _mask_handle(self, mask) if mask is not None else None, vp(d_queries), nq, k,
                                                               group_size, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                               vp(d_row_idx), vp(d_dist), vp(d_group_key or None), vp(d_group_rows or None),
                                                               vp(d_n_found or None), vp(d_n_candidates or None), vp(stream or None)))
            return
        _check(_ffi.lib().pqv_topk_grouped_device(self._h, _group_handle(keys), _mask_handle(self, mask) if mask is not None else None,
                                                  vp(d_queries), nq, k, group_size, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                  vp(d_row_idx), vp(d_dist), vp(d_group_key or None), vp(d_group_rows or None),
                                                  vp(d_n_found or None), vp(d_n_candidates or None), vp(stream or None)))

    def range_search(self, queries, radius, nprobe, max_candidates=0, max_results=0, metric=_ffi.PQV_L2SQ_REF4,
                     sqrt_out=True, mask=None, keys=None, query_keys=None, query_key_ranges=None, query_key_sets=None):
        """Every candidate within `radius` of each query (pqv.h: pqv_range_search), ascending by (d2, candidate position).
        mask / keys + query_keys / query_key_ranges / query_key_sets: as topk (pqv.h: pqv_range_search_masked,
        pqv_range_search_keyed, pqv_range_search_filtered).
        Returns (lims u64 [nq+1], rows u32, dist f32, n_within u64 [nq], n_candidates u64 [nq]): query q's hits are
        rows / dist [lims[q]:lims[q+1]]; n_within is the hit count before max_results."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        radius = float(radius)
        if nprobe == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be > 0")
        if radius != radius:
            raise PqvError(_ffi.PQV_ERR_INVALID, "radius must not be NaN")
        nq, qlen = q.shape
        if qlen != self.dim:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"Query dimension mismatch: expected {self.dim}, got {qlen}")
        nw = np.zeros(nq, dtype=np.uint64)
        nc = np.zeros(nq, dtype=np.uint64)
        lims_p, rows_p, dist_p = u64p(), u32p(), f32p()
        kf = _key_filter(keys, query_keys, query_key_ranges, query_key_sets, nq)
        if kf is not None and kf[0] == "filtered":       # (pqv.h: pqv_range_search_filtered)
            _check(_ffi.lib().pqv_range_search_filtered(self._h, kf[1], C.byref(kf[2]),
                                                        _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                        qlen, radius, nprobe, max_candidates, max_results, metric, 1 if sqrt_out else 0,
                                                        C.byref(lims_p), C.byref(rows_p), C.byref(dist_p), nw.ctypes.data_as(u64p),
                                                        nc.ctypes.data_as(u64p)))
        elif kf is not None:       # (pqv.h: pqv_range_search_keyed)
            kh, qk = kf[1], kf[2]
            _check(_ffi.lib().pqv_range_search_keyed(self._h, kh, qk.ctypes.data_as(_ffi.i64p),
                                                     _mask_handle(self, mask) if mask is not None else None, q.ctypes.data_as(f32p), nq,
                                                     qlen, radius, nprobe, max_candidates, max_results, metric, 1 if sqrt_out else 0,
                                                     C.byref(lims_p), C.byref(rows_p), C.byref(dist_p), nw.ctypes.data_as(u64p),
                                                     nc.ctypes.data_as(u64p)))
        elif mask is not None:       # (pqv.h: pqv_range_search_masked)
            _check(_ffi.lib().pqv_range_search_masked(self._h, _mask_handle(self, mask), q.ctypes.data_as(f32p), nq, qlen, radius, nprobe,
                                                      max_candidates, max_results, metric, 1 if sqrt_out else 0, C.byref(lims_p),
                                                      C.byref(rows_p), C.byref(dist_p), nw.ctypes.data_as(u64p), nc.ctypes.data_as(u64p)))
        else:
            _check(_ffi.lib().pqv_range_search(self._h, q.ctypes.data_as(f32p), nq, qlen, radius, nprobe, max_candidates,
                                               max_results, metric, 1 if sqrt_out else 0, C.byref(lims_p), C.byref(rows_p),
                                               C.byref(dist_p), nw.ctypes.data_as(u64p), nc.ctypes.data_as(u64p)))
        lims, rows, dist = _take_range_buffers(nq, lims_p, rows_p, dist_p)
        return lims, rows, dist, nw, nc

    def range_search_partition(self, queries, radius, part, query_keys=None, query_key_ranges=None, query_key_sets=None, mask=None,
                               max_results=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True):
        """Every row of `part` (a KeyPartition of this searcher) whose key passes the query's filter -- the keywords of
        topk_partition -- within `radius` of the query and within mask if one is given, ascending by (distance, sequence position);
        exact, nothing is probed (pqv.h: pqv_range_search_partition).  Returns (lims u64 [nq+1], rows u32, dist f32, n_within u64
        [nq], n_candidates u64 [nq]) laid out as range_search's."""
        q = _f32(queries)
        if q.ndim == 1:
            q = q.reshape(1, -1)
        nq, qlen = q.shape
        ph, f, _alive = _partition_filter(part, query_keys, query_key_ranges, query_key_sets, nq)
        mh = _mask_handle(self, mask) if mask is not None else None
        radius = float(radius)
        if radius != radius:
            raise PqvError(_ffi.PQV_ERR_INVALID, "radius must not be NaN")
        max_results = int(max_results)
        if max_results < 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "max_results must be >= 0")
        nw = np.zeros(nq, dtype=np.uint64)
        nc = np.zeros(nq, dtype=np.uint64)
        lims_p, rows_p, dist_p = u64p(), u32p(), f32p()
        _check(_ffi.lib().pqv_range_search_partition(self._h, ph, C.byref(f), mh, q.ctypes.data_as(f32p), nq, qlen, radius, max_results,
                                                     metric, 1 if sqrt_out else 0, C.byref(lims_p), C.byref(rows_p), C.byref(dist_p),
                                                     nw.ctypes.data_as(u64p), nc.ctypes.data_as(u64p)))
        lims, rows, dist = _take_range_buffers(nq, lims_p, rows_p, dist_p)
        return lims, rows, dist, nw, nc

    def topk_device(self, d_queries, nq, k, nprobe, d_row_idx, d_dist, d_n_found=0, d_n_candidates=0,
                    max_candidates=0, metric=_ffi.PQV_L2SQ_REF4, sqrt_out=True, stream=0, d_tie_flags=0, mask=None, keys=None,
                    query_keys=None, query_key_ranges=None, query_key_sets=None, max_nprobe=0, d_nprobe_used=0, probe_depths=None,
                    d2_ratio=None):
        """Device-pointer form (ints from tensor.data_ptr()); asynchronous on `stream` -- a hipStream_t handle; 0 means the
        searcher's OWN non-blocking stream, not HIP's / torch's default stream (whose handle is 0 too): work that must follow
        the call on the default stream is NOT ordered behind it, so pass an explicit stream (1 = hipStreamLegacy names the default
        stream itself).  d_tie_flags (u32 [nq]):
        also flag the queries whose answer depends on the reference's heap history (re-submit those to topk()).
        mask (a RowMask of this searcher, alive until the enqueued work has completed): pqv.h: pqv_topk_masked_device.
        keys (a RowKeys of this searcher) with query_keys (the device pointer of int64 [nq], read on `stream` inside the enqueued
        work): pqv.h: pqv_topk_keyed_device; combinable with mask.  Instead of query_keys: query_key_ranges=(ptr_lo, ptr_hi), device
        pointers of int64 [nq] each, or query_key_sets=(ptr_lims, ptr_vals), device pointers of uint64 [nq + 1] offsets and of the
        int64 values, every query's slice strictly ascending and at most PQV_KEY_SET_MAX long -- not validated, the call stays
        asynchronous (pqv.h: pqv_topk_filtered_device).
        max_nprobe (> 0, with mask= or keys=; not with max_candidates): the expanding call, as topk's; d_nprobe_used (u32 [nq],
        optional) takes the lists each query probed (pqv.h: pqv_topk_expand_device).
        probe_depths (the device pointer of uint32 [nq], read on `stream` inside the enqueued work) or d2_ratio (float >= 1), with
        max_nprobe and no filter: per-query probe depths, as topk's; d_nprobe_used as above (pqv.h: pqv_topk_depth_device)."""
        kf = _key_filter(keys, query_keys, query_key_ranges, query_key_sets, nq, device=True)
        if probe_depths is not None or d2_ratio is not None:
            d, _alive = _probe_depth(probe_depths, d2_ratio, max_nprobe or None, max_candidates, mask, kf, nq, device=True)
            _check(_ffi.lib().pqv_topk_depth_device(self._h, C.byref(d), vp(d_queries), nq, k, nprobe, metric, 1 if sqrt_out else 0,
                                                    vp(d_row_idx), vp(d_dist), vp(d_n_found or None), vp(d_n_candidates or None),
                                                    vp(d_nprobe_used or None), vp(d_tie_flags or None), vp(stream or None)))
            return
        if max_nprobe:
            if max_candidates:
                raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe and max_candidates are mutually exclusive")
            kh, fp, _alive = _expand_filter(kf, device=True)
            _check(_ffi.lib().pqv_topk_expand_device(self._h, kh, fp, _mask_handle(self, mask) if mask is not None else None,
                                                     vp(d_queries), nq, k, nprobe, max_nprobe, metric, 1 if sqrt_out else 0,
                                                     vp(d_row_idx), vp(d_dist), vp(d_n_found or None), vp(d_n_candidates or None),
                                                     vp(d_nprobe_used or None), vp(d_tie_flags or None), vp(stream or None)))
            return
        if kf is not None and kf[0] == "filtered":
            _check(_ffi.lib().pqv_topk_filtered_device(self._h, kf[1], C.byref(kf[2]), _mask_handle(self, mask) if mask is not None else None,
                                                       vp(d_queries), nq, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                       vp(d_row_idx), vp(d_dist), vp(d_n_found or None), vp(d_n_candidates or None),
                                                       vp(d_tie_flags or None), vp(stream or None)))
            return
        if kf is not None:
            kh = kf[1]
            _check(_ffi.lib().pqv_topk_keyed_device(self._h, kh, vp(query_keys or None), _mask_handle(self, mask) if mask is not None else None,
                                                    vp(d_queries), nq, k, nprobe, max_candidates, metric, 1 if sqrt_out else 0,
                                                    vp(d_row_idx), vp(d_dist), vp(d_n_found or None), vp(d_n_candidates or None),
                                                    vp(d_tie_flags or None), vp(stream or None)))
            return
        if mask is not None:
            _check(_ffi.lib().pqv_topk_masked_device(self._h, _mask_handle(self, mask), vp(d_queries), nq, k, nprobe, max_candidates,
                                                     metric, 1 if sqrt_out else 0, vp(d_row_idx), vp(d_dist),
                                                     vp(d_n_found or None), vp(d_n_candidates or None), vp(d_tie_flags or None),
                                                     vp(stream or None)))
            return
        if d_tie_flags:
            _check(_ffi.lib().pqv_topk_device_flags(self._h, vp(d_queries), nq, k, nprobe, max_candidates, metric,
                                                    1 if sqrt_out else 0, vp(d_row_idx), vp(d_dist),
                                                    vp(d_n_found or None), vp(d_n_candidates or None), vp(d_tie_flags),
                                                    vp(stream or None)))
            return
        _check(_ffi.lib().pqv_topk_device(self._h, vp(d_queries), nq, k, nprobe, max_candidates, metric,
                                          1 if sqrt_out else 0, vp(d_row_idx), vp(d_dist),
                                          vp(d_n_found or None), vp(d_n_candidates or None),
                                          vp(stream or None)))

    def counters(self):
        c = _ffi.Counters()
        _check(_ffi.lib().pqv_counters(self._h, C.byref(c)))
        return {"queries": c.queries, "candidate_rows": c.candidate_rows,
                "embeddings_fetched": c.embeddings_fetched, "kernel_launches": c.kernel_launches,
                "exact_replays": c.exact_replays, "screened_pairs": c.screened_pairs,
                "screen_survivors": c.screen_survivors}

    def set_option(self, name, value):
        """Force a dispatch choice (pqv.h: pqv_searcher_set_option); results never change."""
        _check(_ffi.lib().pqv_searcher_set_option(self._h, str(name).encode(), int(value)))
        return self

    def describe(self, nq, k, nprobe, metric=_ffi.PQV_L2SQ_REF4):
        buf = C.create_string_buffer(2048)
        _check(_ffi.lib().pqv_searcher_describe(self._h, nq, k, nprobe, metric, buf, len(buf)))
        return buf.value.decode()

    def footprint(self):
        v = [C.c_uint64(0) for _ in range(4)]
        _check(_ffi.lib().pqv_searcher_footprint(self._h, *[C.byref(x) for x in v]))
        return {"row_order_bytes": v[0].value, "ivf_rows_bytes": v[1].value, "blocked_bytes": v[2].value,
                "other_bytes": v[3].value, "total_bytes": sum(x.value for x in v)}

    def set_timing(self, enabled):
        _check(_ffi.lib().pqv_set_timing(self._h, 1 if enabled else 0))

    def timing_read(self):
        rr, tot, n = C.c_double(0), C.c_double(0), C.c_uint32(0)
        _check(_ffi.lib().pqv_timing_read(self._h, C.byref(rr), C.byref(tot), C.byref(n)))
        return rr.value, tot.value, n.value

    def close(self):
        if self._h:
            _ffi.lib().pqv_searcher_free(self._h)
            self._h = None
        for column in self._owned_columns:
            column.close()
        self._owned_columns = []
        self._columns = {}

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_PATH_SEARCHERS = {}
_REALPATHS = {}


def searcher_for_parquet(path, device=0):
    """Index + embedding column of an indexed Parquet file, resident on `device`.  Cached per
    (path, size, mtime): the reference re-opens the file, re-parses the blob and re-reads the
    candidate rows on every query (src/ivf/search.rs:89,102-110); here they stay in HBM."""
    import os
    from . import parquet_io
    st = os.stat(path)
    real = _REALPATHS.get(path)              # (realpath is a handful of system calls: once per spelling of the path)
    if real is None:
        real = _REALPATHS.setdefault(path, os.path.realpath(path))
    key = (real, st.st_size, st.st_mtime_ns, device)
    hit = _PATH_SEARCHERS.get(key)
    if hit is None:
        index, column = parquet_io.read_index_from_parquet(path)
        corpus = parquet_io.load_embedding_column(path, column, device)
        # ONE f32 copy of the column stays resident either way: the images-only IVF layout keeps reading the column as loaded;
        # where the searcher falls back to a list-ordered f32 copy of its own (dim % 64 != 0, short lists, PQV_IVF_COPY=1) the
        # loaded row-order rows are released once that copy exists
        hit = Searcher(index, corpus, _ffi.PQV_LAYOUT_IVF_ORDERED | _ffi.PQV_RELEASE_IF_COPIED)
        _PATH_SEARCHERS.clear()          # one resident file at a time by default
        _PATH_SEARCHERS[key] = hit
    return hit


def _metric_arg(m):
    """The metric of a builder: PQV_L2SQ_REF4 (the default), PQV_COSINE or PQV_DOT (pqv.h: PQV_COSINE, PQV_DOT)."""
    if isinstance(m, bool) or not isinstance(m, int) or m not in (_ffi.PQV_L2SQ_REF4, _ffi.PQV_COSINE, _ffi.PQV_DOT):
        raise PqvError(_ffi.PQV_ERR_INVALID, "unknown metric")
    return int(m)



def _is_expression(x):
    try:
        import pyarrow.compute as pc
    except ImportError:
        return False
    return isinstance(x, pc.Expression)


def _where_arg(x, path, searcher):
    """What .where(x) of a one-file builder accepts: a bool array over the file's rows, a RowMask (searcher sources), or a
    pyarrow.compute.Expression over the file's other columns (path sources).  Returns x checked; anything else is refused."""
    if x is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "where() needs a bool array, a RowMask or a pyarrow expression, got None")
    if isinstance(x, RowMask):
        if searcher is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "where(RowMask) needs a Searcher source: a row mask belongs to one searcher")
        if x._searcher is not searcher:
            raise PqvError(_ffi.PQV_ERR_INVALID, "row mask belongs to another searcher")
        return x
    if _is_expression(x):
        if path is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "where(expression) needs a Parquet path source: the expression is evaluated over the file's columns")
        return x
    if isinstance(x, predicate.Predicate):       # (names resolve at search(): attached columns, or the file's, loaded once)
        return x
    a = np.asarray(x)
    if a.dtype != np.bool_:
        raise PqvError(_ffi.PQV_ERR_INVALID, f"where() needs a bool array, a RowMask or a pyarrow expression, got {a.dtype if a.dtype != object else type(x).__name__}")
    n_rows = searcher._corpus.rows if searcher is not None else _parquet_rows(path)
    return _allow_array(a, n_rows, "where()")


def _parquet_rows(path):
    import pyarrow.parquet as pq
    return pq.ParquetFile(path).metadata.num_rows


def _resolve_where(x, path, searcher):
    """-> (RowMask, owned): the mask of a checked where() argument on `searcher`; owned masks are closed after the search."""
    if isinstance(x, RowMask):
        return x, False
    if isinstance(x, predicate.Predicate):
        if path is not None:
            _attach_file_columns(searcher, path, x.columns())
        return searcher.row_mask_predicate(x), True
    if _is_expression(x):
        from . import parquet_io
        x = parquet_io.row_mask_from_expression(path, x)
    return searcher.row_mask(x), True


def _attach_file_columns(searcher, path, names):
    """The named columns of the searcher's file, resident: loaded on first use and kept with the (cached) searcher, so every later
    predicate over them is device-only."""
    from . import parquet_io
    for name in names:
        if name not in searcher.columns:
            searcher.attach_column(name, parquet_io.load_scalar_column(path, name, searcher._corpus.device), own=True)


def _attach_table_columns(searcher, paths, names):
    """As _attach_file_columns for a table: ONE corpus-row-aligned column per name -- file f's values at its corpus rows, rows
    outside the files NULL; the files must agree on the column's resident type."""
    from . import parquet_io
    for name in names:
        if name in searcher.columns:
            continue
        values = valid = None
        dtype0 = None
        # (a file's rows are its extent, not its index' list rows: a file that had rows removed keeps every row's column value)
        for f, (p, b, n) in enumerate(zip(paths, searcher.row_base.tolist(), searcher.extents.tolist())):
            a, v, dtype = parquet_io.read_scalar_column(p, name)
            if a.size != int(n):
                raise PqvError(_ffi.PQV_ERR_INVALID, f"column {name!r} of file {f} has {a.size} rows, its index has {int(n)}")
            if values is None:
                dtype0 = dtype
                values = np.zeros(searcher._corpus.rows, dtype=a.dtype)
                valid = np.zeros(searcher._corpus.rows, dtype=np.uint8)
            elif dtype != dtype0:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"column {name!r} is {a.dtype} in file {f} and {values.dtype} in file 0: "
                                                     "a table's predicate columns must have one type")
            values[int(b):int(b) + int(n)] = a
            valid[int(b):int(b) + int(n)] = 1 if v is None else v
        searcher.attach_column(name, Column.upload(values, valid, device=searcher._corpus.device), own=True)


def _table_where_arg(x, paths):
    """What .where(x) of a table builder accepts: ONE expression for all files, or one entry per file (bool array or expression)."""
    if x is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "where() needs a pyarrow expression or one bool array / expression per file, got None")
    if isinstance(x, RowMask):
        raise PqvError(_ffi.PQV_ERR_INVALID, "where(RowMask) needs a Searcher source: a row mask belongs to one searcher")
    if _is_expression(x):
        return [x] * len(paths)
    if isinstance(x, predicate.Predicate):       # (ONE predicate for the table: evaluated over corpus-row-aligned columns)
        return x
    if isinstance(x, np.ndarray) or not isinstance(x, (list, tuple)):
        raise PqvError(_ffi.PQV_ERR_INVALID, "a table's where() needs one pyarrow expression, or a list with one bool array / expression per file")
    if len(x) != len(paths):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"where() has {len(x)} entries for {len(paths)} files")
    return [_where_arg(xf, p, None) for xf, p in zip(x, paths)]


def _resolve_table_where(per_file, paths, searcher):
    from . import parquet_io
    if isinstance(per_file, predicate.Predicate):
        _attach_table_columns(searcher, paths, per_file.columns())
        return searcher.row_mask_predicate(per_file)
    allowed = np.zeros(searcher._corpus.rows, dtype=np.uint8)
    for xf, p, b, n in zip(per_file, paths, searcher.row_base.tolist(), searcher.extents.tolist()):
        a = parquet_io.row_mask_from_expression(p, xf) if _is_expression(xf) else xf
        a = _allow_array(a, int(n), "where()")
        allowed[int(b):int(b) + int(n)] = a
    return searcher.row_mask(allowed)


class TopkBuilder:
    """src/ivf/search.rs:49-81: k and nprobe must be set and > 0.  `source` is an indexed
    Parquet path (as in the reference) or an existing Searcher.  metric(m): PQV_L2SQ_REF4 (default, distances
    sqrt(d2) as the reference returns them), PQV_COSINE (0.5 * d2 of the normalised vectors, pqv.h: PQV_COSINE) or PQV_DOT (the negated
    inner product -(q.x), smallest first, pqv.h: PQV_DOT; not with distinct_on)."""

    def __init__(self, source, query, device=0):
        import os
        if isinstance(source, (str, bytes, os.PathLike)):
            self._path, self._searcher = source, None
        else:
            self._path, self._searcher = None, source
        self._device = device
        self._query = query
        self._k = None
        self._nprobe = None
        self._metric = _ffi.PQV_L2SQ_REF4
        self._where = None
        self._distinct = None
        self._group_size = None
        self._max_nprobe = None
        self._d2_ratio = None
        self._mmr = None

    def mmr(self, fetch_k, lambda_=0.5):
        """Diversify the result: fetch the fetch_k (>= k) nearest rows, then pick k of them by maximal marginal relevance with weight
        lambda_ in [0, 1] on the distance to the query (pqv.h: pqv_topk_mmr).  search() returns the picks in pick order.  Composes
        with where() and metric(); not with distinct_on(), max_nprobe() or d2_ratio(): diversify their results with
        Searcher.mmr_select."""
        if fetch_k == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "fetch_k must be > 0")
        if not 0.0 <= lambda_ <= 1.0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "lambda must be in [0, 1]")
        self._mmr = (fetch_k, float(lambda_))
        return self

    def _check_mmr(self):
        if self._mmr is None:
            return
        if self._distinct is not None:
            raise PqvError(_ffi.PQV_ERR_UNSUPPORTED, "mmr() does not combine with distinct_on(): pick among a distinct call's rows with "
                                                     "Searcher.mmr_select (pqv.h: pqv_mmr_select)")
        if self._max_nprobe is not None or self._d2_ratio is not None:
            raise PqvError(_ffi.PQV_ERR_UNSUPPORTED, "mmr() does not combine with max_nprobe() or d2_ratio(): pick among their rows with "
                                                     "Searcher.mmr_select (pqv.h: pqv_mmr_select)")

    def max_nprobe(self, n):
        """With where(): keep probing, up to n lists, until k rows pass the filter (pqv.h: pqv_topk_expand); nprobe() stays the
        fewest lists probed.  Not with distinct_on(); table builders do not take it.  With d2_ratio(): the ceiling of the depth."""
        if n == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "max_nprobe must be > 0")
        self._max_nprobe = n
        return self

    def d2_ratio(self, r):
        """With max_nprobe(n) and no where() / distinct_on(): probe the lists whose centroid is within r (>= 1, squared scale) of the
        nearest centroid's distance, at least nprobe() and at most n of them (pqv.h: pqv_topk_depth)."""
        if not r >= 1.0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "d2_ratio must be >= 1 and not NaN")
        self._d2_ratio = float(r)
        return self

    def metric(self, m):
        self._metric = _metric_arg(m)
        return self

    def distinct_on(self, x):
        """`SELECT DISTINCT ON (x) .. ORDER BY distance LIMIT k`: the nearest row of each of the k nearest values of an integer
        column -- the k nearest documents, not k chunks of one (pqv.h: pqv_topk_distinct).  x: the name of an integer column (with a
        path source the file's, loaded once per resident file; with a Searcher source an attached one), or a RowKeys of the
        searcher.  Rows whose value is NULL belong to no group.  search() then returns [DistinctSearchResult(row_idx, distance,
        key)]; composes with where() and metric()."""
        if isinstance(x, RowKeys):
            if self._searcher is None:
                raise PqvError(_ffi.PQV_ERR_INVALID, "distinct_on(RowKeys) needs a Searcher source: row keys belong to one searcher")
        elif not isinstance(x, str):
            raise PqvError(_ffi.PQV_ERR_INVALID, f"distinct_on() needs a column name or a RowKeys, got {type(x).__name__}")
        self._distinct = x
        return self

    def group_size(self, m):
        """With distinct_on(x): up to m rows of each of the k nearest values of x -- the k nearest documents and the m best chunks of
        each (pqv.h: pqv_topk_grouped).  search() then returns [GroupSearchResult(key, hits=[SearchResult])], groups nearest first,
        a group's hits nearest first.  Without distinct_on() search() raises."""
        if m == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "group_size must be > 0")
        self._group_size = m
        return self

    def _search_grouped(self, searcher, mask, max_candidates=0, max_nprobe=None):
        """-> [(key, rows, dist)] of the found groups."""
        keys, owned = self._group_keys(searcher)
        try:
            rows, dist, grp, grows, nf = searcher.topk_grouped(_f32(self._query).reshape(1, -1), self._k, self._group_size, self._nprobe,
                                                               keys, mask=mask, max_candidates=max_candidates, metric=self._metric,
                                                               max_nprobe=max_nprobe)[:5]
        finally:
            if owned:
                keys.close()
        return [(int(grp[0, g]), rows[0, g, :int(grows[0, g])], dist[0, g, :int(grows[0, g])]) for g in range(int(nf[0]))]

    def _check_grouping(self):
        if self._group_size is not None and self._distinct is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "group_size() needs distinct_on(): the column whose values are the groups")

    def _group_keys(self, searcher):
        """-> (RowKeys, owned) of the distinct_on() argument on `searcher`."""
        if isinstance(self._distinct, RowKeys):
            return self._distinct, False
        if self._path is not None:
            _attach_file_columns(searcher, self._path, [self._distinct])
        return searcher.row_keys(self._distinct), True

    def _search_distinct(self, searcher, mask, max_candidates=0, max_nprobe=None):
        keys, owned = self._group_keys(searcher)
        try:
            rows, dist, grp, nf = searcher.topk_distinct(_f32(self._query).reshape(1, -1), self._k, self._nprobe, keys, mask=mask,
                                                         max_candidates=max_candidates, metric=self._metric, max_nprobe=max_nprobe)[:4]
        finally:
            if owned:
                keys.close()
        n = int(nf[0])
        return rows[0, :n], dist[0, :n], grp[0, :n]

    def where(self, x):
        """Restrict the search to rows (the reference's `WHERE <predicate>` inside the scan, exec.rs:207-277): a bool array over
        the file's rows, a RowMask (Searcher sources), a pyarrow.compute.Expression over the file's other columns, e.g.
        pc.field("id") >= 2 (path sources; evaluated on the host; nulls count as False), or a predicate, e.g. pqv.col("id") >= 2,
        evaluated on the GPU over resident columns: the searcher's attached columns, or with a path source the file's columns,
        loaded once per resident file.  Fewer than k rows may come back."""
        self._where = _where_arg(x, self._path, self._searcher)
        return self

    def k(self, k):
        if k == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "k must be > 0")
        self._k = k
        return self

    def nprobe(self, nprobe):
        if nprobe == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be > 0")
        self._nprobe = nprobe
        return self

    def search(self):
        if self._k is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "k must be set")
        if self._nprobe is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be set")
        self._check_grouping()
        self._check_mmr()
        if self._d2_ratio is not None:
            if self._max_nprobe is None:
                raise PqvError(_ffi.PQV_ERR_INVALID, "probe_depths / d2_ratio need max_nprobe")
            if self._where is not None or self._distinct is not None:
                raise PqvError(_ffi.PQV_ERR_UNSUPPORTED, "d2_ratio() does not combine with where() or distinct_on() (pqv.h: pqv_topk_depth)")
        elif self._max_nprobe is not None and self._where is None and self._distinct is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "pqv_topk_expand needs a row mask or row keys")
        if self._searcher is None:
            self._searcher = searcher_for_parquet(self._path, self._device)
        if self._distinct is not None:
            mask, owned = _resolve_where(self._where, self._path, self._searcher) if self._where is not None else (None, False)
            try:
                if self._group_size is not None:
                    return [GroupSearchResult(g, [SearchResult(r, d) for r, d in zip(rows.tolist(), dist.tolist())])
                            for g, rows, dist in self._search_grouped(self._searcher, mask, max_nprobe=self._max_nprobe)]
                rows, dist, grp = self._search_distinct(self._searcher, mask, max_nprobe=self._max_nprobe)
            finally:
                if owned:
                    mask.close()
            return [DistinctSearchResult(r, d, g) for r, d, g in zip(rows.tolist(), dist.tolist(), grp.tolist())]
        if self._mmr is not None:
            mask, owned = _resolve_where(self._where, self._path, self._searcher) if self._where is not None else (None, False)
            try:
                rows, dist, _, nf, _ = self._searcher.topk_mmr(_f32(self._query).reshape(1, -1), self._k, self._mmr[0], self._nprobe,
                                                               lambda_=self._mmr[1], mask=mask, metric=self._metric)
            finally:
                if owned:
                    mask.close()
        elif self._where is not None:
            mask, owned = _resolve_where(self._where, self._path, self._searcher)
            try:
                rows, dist, nf = self._searcher.topk(_f32(self._query).reshape(1, -1), self._k, self._nprobe, metric=self._metric,
                                                     mask=mask, max_nprobe=self._max_nprobe)[:3]
            finally:
                if owned:
                    mask.close()
        elif self._d2_ratio is not None:
            rows, dist, nf = self._searcher.topk(_f32(self._query).reshape(1, -1), self._k, self._nprobe, metric=self._metric,
                                                 max_nprobe=self._max_nprobe, d2_ratio=self._d2_ratio)[:3]
        else:
            rows, dist, nf, _ = self._searcher.topk(_f32(self._query).reshape(1, -1), self._k, self._nprobe, metric=self._metric)
        n = int(nf[0])
        return [SearchResult(r, d) for r, d in zip(rows[0, :n].tolist(), dist[0, :n].tolist())]


class RangeBuilder:
    """Range counterpart of TopkBuilder: every row within `radius` of the query, nearest first (ties by candidate
    position).  radius and nprobe must be set; max_results (optional, > 0) keeps the first that many.  `source` is an
    indexed Parquet path or an existing Searcher.  metric(m): as TopkBuilder's (PQV_COSINE: radius on the 0.5 * d2 scale; PQV_DOT: hits have
    -(q.x) <= radius, so radius = -0.8 keeps q.x >= 0.8)."""

    def __init__(self, source, query, device=0):
        import os
        if isinstance(source, (str, bytes, os.PathLike)):
            self._path, self._searcher = source, None
        else:
            self._path, self._searcher = None, source
        self._device = device
        self._query = query
        self._radius = None
        self._nprobe = None
        self._max_results = 0
        self._metric = _ffi.PQV_L2SQ_REF4
        self._where = None

    def metric(self, m):
        self._metric = _metric_arg(m)
        return self

    def where(self, x):
        """As TopkBuilder.where: only rows that pass are hits."""
        self._where = _where_arg(x, self._path, self._searcher)
        return self

    def radius(self, radius):
        radius = float(radius)
        if radius != radius:
            raise PqvError(_ffi.PQV_ERR_INVALID, "radius must not be NaN")
        self._radius = radius
        return self

    def nprobe(self, nprobe):
        if nprobe == 0:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be > 0")
        self._nprobe = nprobe
        return self

    def max_results(self, max_results):
        self._max_results = int(max_results)
        return self

    def search(self):
        if self._radius is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "radius must be set")
        if self._nprobe is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be set")
        if self._searcher is None:
            self._searcher = searcher_for_parquet(self._path, self._device)
        if self._where is not None:
            mask, owned = _resolve_where(self._where, self._path, self._searcher)
            try:
                _, rows, dist, _, _ = self._searcher.range_search(_f32(self._query).reshape(1, -1), self._radius, self._nprobe,
                                                                  max_results=self._max_results, metric=self._metric, mask=mask)
            finally:
                if owned:
                    mask.close()
        else:
            _, rows, dist, _, _ = self._searcher.range_search(_f32(self._query).reshape(1, -1), self._radius, self._nprobe,
                                                              max_results=self._max_results, metric=self._metric)
        return [SearchResult(r, d) for r, d in zip(rows.tolist(), dist.tolist())]


# ---------------------------------------------------------------------------------------
# A table of indexed files on one GPU (pqv.h: pqv_table_searcher_create; src/df_vector/index_exec.rs:85-164, exec.rs:264-267)
@dataclass
class TableSearchResult:
    """One row of the reference's index scan over a table: the file it came from, its row id in that file, the distance."""
    path: str
    row_idx: int
    distance: float


@dataclass
class TableDistinctSearchResult:
    """TableSearchResult of a distinct top-k (TableTopkBuilder.distinct_on), with the group's key value."""
    path: str
    row_idx: int
    distance: float
    key: int


def _table_args(indexes, corpus, row_base):
    """Host-side checks of a table (the library repeats them): returned as (indexes, row_base u64 array)."""
    indexes = list(indexes)
    if not indexes:
        raise PqvError(_ffi.PQV_ERR_INVALID, "a table needs at least one indexed file")
    if corpus is None:
        raise PqvError(_ffi.PQV_ERR_INVALID, "indexes/row_base/corpus must not be NULL")
    rb = np.ascontiguousarray(row_base, dtype=np.uint64).reshape(-1)
    if rb.size != len(indexes):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"row_base has {rb.size} entries for {len(indexes)} files")
    dim0, end = indexes[0].dim, 0
    for f, ix in enumerate(indexes):
        if ix.dim != dim0:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"index dimension {ix.dim} of file {f} does not match dimension {dim0} of file 0")
        if ix.dim != corpus.dim:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"index dimension {ix.dim} of file {f} does not match corpus dimension {corpus.dim}")
        b, n = int(rb[f]), ix.row_bound          # the file's extent: ids a remove left free stay the file's
        if f > 0 and b < end:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"row range of file {f} starts at {b}, inside the rows of the files before it "
                                                 "(ranges must be increasing and disjoint)")
        if b + n > corpus.rows:
            raise PqvError(_ffi.PQV_ERR_INVALID, f"row range [{b}, {b + n}) of file {f} lies outside the corpus of {corpus.rows} rows")
        end = b + n
    if end >= 0xFFFFFFFF:
        raise PqvError(_ffi.PQV_ERR_INVALID, "a table's rows must stay below 2^32 - 1 (0xFFFFFFFF marks an empty slot)")
    return indexes, rb


class TableSearcher(Searcher):
    """Several indexed files searched as ONE table on one GPU: file f's rows are corpus rows [row_base[f], row_base[f] + its
    extent), the extent being its index' row bound: its row count until a remove, after which the ids run on up to the bound
    (n_rows keeps the files' list rows, extents their bounds).  nprobe counts per file; probe() returns the P = sum_f
    min(nprobe, kc_f) global list ids, file after file; rows come back as corpus rows (split_rows maps them to (file, local
    row), by the extents).  max_candidates > 0 needs
    flags |= PQV_TABLE_CAP_ROUND_ROBIN: file f then considers the first round_robin_quota(its candidate counts, max_candidates)[f]
    of its candidates, as the reference's CandidateCursor deals them; without the flag it is refused (PQV_ERR_UNSUPPORTED)."""

    def __init__(self, indexes, corpus, row_base, flags=_ffi.PQV_LAYOUT_IVF_ORDERED):
        indexes, rb = _table_args(indexes, corpus, row_base)
        arr = (vp * len(indexes))(*[ix._h for ix in indexes])
        h = vp()
        _check(_ffi.lib().pqv_table_searcher_create(arr, len(indexes), rb.ctypes.data_as(u64p), corpus._h, flags, C.byref(h)))
        self._h = h
        self._corpus = corpus
        self._columns = {}
        self._owned_columns = []
        self.dim = indexes[0].dim
        self.n_clusters = sum(ix.n_clusters for ix in indexes)
        self.n_files = len(indexes)
        self.row_base = rb.copy()
        self.n_rows = np.array([ix.n_rows for ix in indexes], dtype=np.uint64)          # list rows of each file
        self.extents = np.array([ix.row_bound for ix in indexes], dtype=np.uint64)      # the files' local ids run below these
        self.cluster_base = np.concatenate([[0], np.cumsum([ix.n_clusters for ix in indexes])]).astype(np.uint32)

    _extents = None

    @property
    def extents(self):
        """u64 [n_files]: the rows of each file as the table sees them -- its index' row bound; for files read from Parquet
        (searcher_for_parquet_files) the file's row count, which is at least that.  n_rows where none were given: the two are
        equal until rows are removed."""
        return self.n_rows if self._extents is None else self._extents

    @extents.setter
    def extents(self, value):
        self._extents = np.asarray(value, dtype=np.uint64).reshape(-1)

    def probe_count(self, nprobe):
        """P: the lists one query probes (the sum over the files of min(nprobe, kc_f))."""
        return int(np.minimum(np.diff(self.cluster_base.astype(np.int64)), int(nprobe)).sum())

    def probe(self, query, nprobe):
        q = _f32(query).reshape(-1)
        out = np.zeros(max(1, self.probe_count(nprobe)), dtype=np.uint32)
        n = C.c_uint32(0)
        _check(_ffi.lib().pqv_probe(self._h, q.ctypes.data_as(f32p), q.size, nprobe,
                                    out.ctypes.data_as(u32p), C.byref(n)))
        return out[:n.value].copy()

    def split_rows(self, rows):
        """Corpus rows -> (file, local row) arrays (0xFFFFFFFF, an empty slot, maps to file -1)."""
        return split_table_rows(rows, self.row_base, self.extents)


def split_table_rows(rows, row_base, n_rows=None):
    """Corpus rows of a table -> (file index int64, row in that file u32); rows outside every file (and 0xFFFFFFFF) give file
    -1.  row_base: increasing first rows of the files; n_rows: their extents -- the row counts, or the row bounds where rows were
    removed (default: up to the next file's base)."""
    rows = np.asarray(rows, dtype=np.uint64)
    rb = np.asarray(row_base, dtype=np.uint64).reshape(-1)
    f = np.searchsorted(rb, rows, side="right").astype(np.int64) - 1
    fi = np.clip(f, 0, max(0, rb.size - 1))
    local = rows - rb[fi] if rb.size else rows
    ok = (f >= 0) & (rows != 0xFFFFFFFF)
    if n_rows is not None:
        ok &= local < np.asarray(n_rows, dtype=np.uint64).reshape(-1)[fi]
    return np.where(ok, f, -1), np.where(ok, local, 0xFFFFFFFF).astype(np.uint32)


def round_robin_quota(counts, max_candidates):
    """What CandidateCursor::next_batch(max_candidates) of a fresh cursor takes from each file (access.rs:214-242), given the
    files' candidate counts: u64 [n_files].  max_candidates == 0: no cap (the counts themselves)."""
    c = np.ascontiguousarray(counts, dtype=np.uint64).reshape(-1)
    out = np.zeros(max(1, c.size), dtype=np.uint64)
    _check(_ffi.lib().pqv_round_robin_quota(c.ctypes.data_as(u64p), c.size, int(max_candidates), out.ctypes.data_as(u64p)))
    return out[:c.size]


def _max_candidates_arg(n):
    """A builder's max_candidates: an integer in [1, 2^64) (VectorTopKOptions::max_candidates; None there = no cap)."""
    if isinstance(n, (bool, np.bool_)) or not isinstance(n, (int, np.integer)):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"max_candidates must be an integer, got {type(n).__name__}")
    if not 0 < int(n) < (1 << 64):
        raise PqvError(_ffi.PQV_ERR_INVALID, f"max_candidates must be in [1, 2^64), got {int(n)}")
    return int(n)


_TABLE_SEARCHERS = {}


def searcher_for_parquet_files(paths, device=0, round_robin_cap=False):
    """A TableSearcher over indexed Parquet files: every file's index blob and embedding column, the columns loaded one after
    the other into ONE resident corpus.  Cached per (files, sizes, mtimes, device, round_robin_cap) as searcher_for_parquet is.
    round_robin_cap: created with PQV_TABLE_CAP_ROUND_ROBIN (max_candidates allowed, dealt out round robin over the files)."""
    import os
    from . import parquet_io
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    paths = list(paths)
    if not paths:
        raise PqvError(_ffi.PQV_ERR_INVALID, "a table needs at least one indexed file")
    key = []
    for p in paths:
        st = os.stat(p)
        real = _REALPATHS.get(p)
        if real is None:
            real = _REALPATHS.setdefault(p, os.path.realpath(p))
        key.append((real, st.st_size, st.st_mtime_ns))
    key = (tuple(key), device, bool(round_robin_cap))
    hit = _TABLE_SEARCHERS.get(key)
    if hit is None:
        import pyarrow.parquet as pq
        parts = [parquet_io.read_index_from_parquet(p) for p in paths]
        indexes = [ix for ix, _ in parts]
        dim0 = indexes[0].dim
        for f, ix in enumerate(indexes):
            if ix.dim != dim0:
                raise PqvError(_ffi.PQV_ERR_INVALID, f"index dimension {ix.dim} of file {f} does not match dimension {dim0} of file 0")
        counts = [pq.ParquetFile(p).metadata.num_rows for p in paths]
        row_base = np.concatenate([[0], np.cumsum(counts)[:-1]]).astype(np.uint64)
        total = int(sum(counts))
        if total >= 0xFFFFFFFF:
            raise PqvError(_ffi.PQV_ERR_INVALID, "a table's rows must stay below 2^32 - 1 (0xFFFFFFFF marks an empty slot)")
        corpus = Corpus.create(total, dim0, device)
        try:
            for p, (_, column), b in zip(paths, parts, row_base):
                parquet_io.load_embedding_column(p, column, device, into=corpus, row_offset=int(b))
            corpus.finish(total)
            flags = _ffi.PQV_LAYOUT_IVF_ORDERED | _ffi.PQV_RELEASE_IF_COPIED
            if round_robin_cap:
                flags |= _ffi.PQV_TABLE_CAP_ROUND_ROBIN
            hit = TableSearcher(indexes, corpus, row_base, flags)
            hit.extents = counts          # (a file's rows: at least its index' row bound, more where its newest rows were removed)
        except Exception:
            corpus.close()
            raise
        hit.paths = [str(p) for p in paths]
        _TABLE_SEARCHERS.clear()
        _TABLE_SEARCHERS[key] = hit
    return hit


def _table_paths(paths):
    import os
    if isinstance(paths, (str, bytes, os.PathLike)):
        paths = [paths]
    paths = list(paths)
    if not paths:
        raise PqvError(_ffi.PQV_ERR_INVALID, "a table needs at least one indexed file")
    return paths


def _table_results(searcher, paths, rows, dist):
    f, local = searcher.split_rows(rows)
    return [TableSearchResult(str(paths[int(i)]), int(r), float(d)) for i, r, d in zip(f.tolist(), local.tolist(), dist.tolist())]


class TableTopkBuilder(TopkBuilder):
    """TopkBuilder over a table of indexed Parquet files (searched as one TableSearcher; nprobe per file).  search() returns
    [TableSearchResult(path, row_idx, distance)] -- the (path, row id, distance) columns of the reference's index scan.
    max_candidates(n): VectorTopKOptions::max_candidates -- n candidates dealt out round robin over the files (exec.rs:207-245)."""

    def __init__(self, paths, query, device=0):
        self._paths = _table_paths(paths)
        self._max_candidates = 0
        super().__init__(None, query, device)

    def max_candidates(self, n):
        self._max_candidates = _max_candidates_arg(n)
        return self

    def where(self, x):
        """One pyarrow expression or one predicate (pqv.col(...), evaluated on the GPU) for all files, or a list with one bool array /
        expression per file (TopkBuilder.where)."""
        self._where = _table_where_arg(x, self._paths)
        return self

    def distinct_on(self, x):
        """TopkBuilder.distinct_on over the table: x names an integer column that every file has (one resident type); search()
        returns [TableDistinctSearchResult(path, row_idx, distance, key)], with group_size(m) [GroupSearchResult(key,
        hits=[TableSearchResult])]."""
        if not isinstance(x, str):
            raise PqvError(_ffi.PQV_ERR_INVALID, f"a table's distinct_on() needs a column name, got {type(x).__name__}")
        self._distinct = x
        return self

    def _group_keys(self, searcher):
        _attach_table_columns(searcher, self._paths, [self._distinct])
        return searcher.row_keys(self._distinct), True

    def search(self):
        if self._k is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "k must be set")
        if self._nprobe is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be set")
        self._check_grouping()
        if self._max_nprobe is not None:
            raise PqvError(_ffi.PQV_ERR_UNSUPPORTED, "pqv_topk_expand does not take table searchers")
        if self._mmr is not None:
            raise PqvError(_ffi.PQV_ERR_UNSUPPORTED, "pqv_topk_mmr does not take table searchers")
        s = searcher_for_parquet_files(self._paths, self._device, round_robin_cap=self._max_candidates > 0)
        if self._distinct is not None:
            mask = _resolve_table_where(self._where, self._paths, s) if self._where is not None else None
            try:
                if self._group_size is not None:
                    return [GroupSearchResult(g, _table_results(s, self._paths, rows, dist))
                            for g, rows, dist in self._search_grouped(s, mask, self._max_candidates)]
                rows, dist, grp = self._search_distinct(s, mask, self._max_candidates)
            finally:
                if mask is not None:
                    mask.close()
            return [TableDistinctSearchResult(r.path, r.row_idx, r.distance, int(g))
                    for r, g in zip(_table_results(s, self._paths, rows, dist), grp.tolist())]
        if self._where is not None:
            mask = _resolve_table_where(self._where, self._paths, s)
            try:
                rows, dist, nf, _ = s.topk(_f32(self._query).reshape(1, -1), self._k, self._nprobe, max_candidates=self._max_candidates,
                                           metric=self._metric, mask=mask)
            finally:
                mask.close()
        else:
            rows, dist, nf, _ = s.topk(_f32(self._query).reshape(1, -1), self._k, self._nprobe, max_candidates=self._max_candidates,
                                       metric=self._metric)
        n = int(nf[0])
        return _table_results(s, self._paths, rows[0, :n], dist[0, :n])


class TableRangeBuilder(RangeBuilder):
    """RangeBuilder over a table of indexed Parquet files; search() returns [TableSearchResult], nearest first.
    max_candidates(n): as TableTopkBuilder's."""

    def __init__(self, paths, query, device=0):
        self._paths = _table_paths(paths)
        self._max_candidates = 0
        super().__init__(None, query, device)

    def max_candidates(self, n):
        self._max_candidates = _max_candidates_arg(n)
        return self

    def where(self, x):
        """As TableTopkBuilder.where."""
        self._where = _table_where_arg(x, self._paths)
        return self

    def search(self):
        if self._radius is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "radius must be set")
        if self._nprobe is None:
            raise PqvError(_ffi.PQV_ERR_INVALID, "nprobe must be set")
        s = searcher_for_parquet_files(self._paths, self._device, round_robin_cap=self._max_candidates > 0)
        if self._where is not None:
            mask = _resolve_table_where(self._where, self._paths, s)
            try:
                _, rows, dist, _, _ = s.range_search(_f32(self._query).reshape(1, -1), self._radius, self._nprobe,
                                                     max_candidates=self._max_candidates, max_results=self._max_results,
                                                     metric=self._metric, mask=mask)
            finally:
                mask.close()
        else:
            _, rows, dist, _, _ = s.range_search(_f32(self._query).reshape(1, -1), self._radius, self._nprobe,
                                                 max_candidates=self._max_candidates, max_results=self._max_results, metric=self._metric)
        return _table_results(s, self._paths, rows, dist)


# ---------------------------------------------------------------------------------------
def rerank_batch(query, cand, k, state=None, ids=None, valid=None, metric=_ffi.PQV_L2SQ_SEQ, device=0):
    """update_topk_heap for one RecordBatch (src/df_vector/exec.rs:457-484).

    state = (rows u32[<=k], d2 f32[<=k]): the reference heap's backing array after the previous batch (None for the
    first); returns the new state.  A float64 `cand` is narrowed `as f32` by the library (exec.rs:538-545).
    rerank_finish(state) gives the rows in output order."""
    q = _f32(query).reshape(-1)
    cand = np.asarray(cand)
    f64 = cand.dtype == np.float64
    cand = np.ascontiguousarray(cand, dtype=np.float64 if f64 else np.float32)
    m, dim = cand.shape if cand.ndim == 2 else (0, q.size)
    io_rows = np.zeros(max(k, 1), dtype=np.uint32)
    io_d2 = np.zeros(max(k, 1), dtype=np.float32)
    cnt = C.c_uint32(0)
    if state is not None:
        r, d = state
        cnt.value = len(r)
        io_rows[:len(r)] = r
        io_d2[:len(r)] = d
    ids_a = None if ids is None else np.ascontiguousarray(ids, dtype=np.uint32)
    valid_a = None if valid is None else np.ascontiguousarray(valid, dtype=np.uint8)
    fn = _ffi.lib().pqv_rerank_f64 if f64 else _ffi.lib().pqv_rerank
    _check(fn(device, q.ctypes.data_as(f32p), cand.ctypes.data_as(_ffi.f64p if f64 else f32p),
              None if ids_a is None else ids_a.ctypes.data_as(u32p),
              None if valid_a is None else valid_a.ctypes.data_as(u8p),
              m, dim, k, metric, io_rows.ctypes.data_as(u32p),
              io_d2.ctypes.data_as(f32p), C.byref(cnt)))
    return io_rows[:cnt.value].copy(), io_d2[:cnt.value].copy()


def rerank_finish(state):
    """heap.into_iter() + the stable sort by distance (src/df_vector/exec.rs:269-274): (rows, d2) ascending."""
    r = np.ascontiguousarray(state[0], dtype=np.uint32)
    d = np.ascontiguousarray(state[1], dtype=np.float32)
    orow = np.empty(max(len(r), 1), dtype=np.uint32)
    od = np.empty(max(len(r), 1), dtype=np.float32)
    _check(_ffi.lib().pqv_rerank_finish(r.ctypes.data_as(u32p), d.ctypes.data_as(f32p), len(r),
                                        orow.ctypes.data_as(u32p), od.ctypes.data_as(f32p)))
    return orow[:len(r)], od[:len(r)]


def merge_topk(dist, rows, counts):
    """Merge per-shard lists [n_lists, nq, k] -> (dist [nq,k], rows [nq,k], list [nq,k], count [nq])."""
    dist = _f32(dist)
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    counts = np.ascontiguousarray(counts, dtype=np.uint32)
    n_lists, nq, k = dist.shape
    od = np.empty((nq, k), dtype=np.float32)
    orow = np.empty((nq, k), dtype=np.uint32)
    ol = np.empty((nq, k), dtype=np.uint32)
    oc = np.empty(nq, dtype=np.uint32)
    _check(_ffi.lib().pqv_merge_topk(dist.ctypes.data_as(f32p), rows.ctypes.data_as(u32p),
                                     counts.ctypes.data_as(u32p), n_lists, nq, k,
                                     od.ctypes.data_as(f32p), orow.ctypes.data_as(u32p),
                                     ol.ctypes.data_as(u32p), oc.ctypes.data_as(u32p)))
    return od, orow, ol, oc
