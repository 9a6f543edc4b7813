"""pq_vector_amd -- MI355X-native IVF index build + top-k search (pq-vector's hot path).

Host-side mirror of the reference's Rust API over the C ABI of include/pqv.h:

    reference (Rust)                         here
    ---------------------------------------  -------------------------------------------
    IndexBuilder::new(src, col)              IndexBuilder(source[, embedding_column])
      .n_clusters(n).max_iters(m).seed(s)      .n_clusters(n).max_iters(m).seed(s)
      .build_inplace() / .build_new(out)       .build() -> Index   (in-memory form)
    TopkBuilder::new(path, &query)           TopkBuilder(searcher, query)
      .k(k)?.nprobe(n)?.search().await?        .k(k).nprobe(n).search() -> [SearchResult]
    SearchResult{row_idx, distance}          SearchResult(row_idx, distance)
    (no counterpart: range search)           RangeBuilder(searcher, query).radius(r).nprobe(n).search()
    index scan over a table of files         TableTopkBuilder(paths, query).k(k).nprobe(n).search()
      (df_vector/index_exec.rs:85-164)         -> [TableSearchResult(path, row_idx, distance)]
    VectorTopKOptions{max_candidates: Some(m)} TableTopkBuilder(...).max_candidates(m) (round robin over the files)
    WHERE tenant = ? / ts BETWEEN ? AND ? /  Searcher.row_keys(column) + topk / range_search / topk_device (keys=..., and one of
      grp IN (...), one filter PER QUERY       query_keys= / query_key_ranges=(lo, hi) / query_key_sets=[...])
    WHERE <predicate> inside the scan        every builder: .where(bool array | RowMask | pyarrow expression | predicate);
      (df_vector/exec.rs:207-277)              Searcher.row_mask(allowed) + topk / range_search / topk_device (mask=...)
                                               predicates (col("id") >= 2, & | ~) run on the GPU over resident Columns
    (no counterpart: probe on until k rows   topk / topk_device (mask= or keys=..., max_nprobe=P) -> also nprobe_used [nq];
      pass the filter)                         TopkBuilder(...).where(...).max_nprobe(P)
    (no counterpart: a probe depth per       topk / topk_device (probe_depths=... | d2_ratio=r, max_nprobe=P) -> also nprobe_used [nq];
      query of the plain call)                 TopkBuilder(...).d2_ratio(r).max_nprobe(P)
    SELECT DISTINCT ON (doc) .. LIMIT k      TopkBuilder / TableTopkBuilder: .distinct_on("doc") -> [DistinctSearchResult(row_idx,
      (no counterpart: grouping)               distance, key)]; Searcher.topk_distinct / topk_distinct_device (keys=RowKeys)
    ROW_NUMBER() OVER (PARTITION BY doc      .distinct_on("doc").group_size(m) -> [GroupSearchResult(key, hits=[SearchResult])]: up to m
      ORDER BY distance) <= m, k docs          rows of each of the k nearest groups; Searcher.topk_grouped / topk_grouped_device
    (no counterpart: a posting list per      Searcher.key_partition(column) + topk_partition / topk_partition_grouped (exact top-k over a
      tenant, nothing probed)                  tenant's own rows) / range_search_partition (every row of the tenant within a radius)
    WHERE id IN (rows another engine named,  Searcher.topk_rows(queries, k, candidates) (the exact top-k among exactly those rows, a list per
      per query: hybrid retrieval)             query) / score_rows (every candidate's exact distance); topk_rows_device / score_rows_device
    (no counterpart: MMR, k diverse rows     Searcher.topk_mmr(queries, k, fetch_k, nprobe, lambda_) / TopkBuilder(...).mmr(fetch_k, lambda_);
      out of the fetch_k nearest)              Searcher.mmr_select(rows, dist, k) over any call's [nq, n] result; the _device forms
    (no counterpart: rows that arrive after  corpus.append(batch); index = index.append(corpus) -> a new Index, same centroids, every
      the build; indexing under a given        list extended (no k-means); Index.assign(corpus, first_row, n_rows);
      codebook)                                IndexBuilder(source).with_centroids(index_or_array).build()

(src/ivf/parquet.rs:23-103, src/ivf/search.rs:41-81).  All compute runs in the HIP kernels
behind libpqv_hip.so; importing this package without the built library fails loudly.
"""
from .api import (CandidateCursor, Column, Corpus, DistinctSearchResult, GroupSearchResult, TableDistinctSearchResult, Index, IndexBuilder, PqvError, RangeBuilder, KeyPartition, RowKeys, RowMask, Searcher, SearchResult, TopkBuilder,
                  TableRangeBuilder, TableSearcher, TableSearchResult, TableTopkBuilder, device_count, merge_topk, rerank_batch,
                  rerank_finish, round_robin_quota, searcher_for_parquet, searcher_for_parquet_files, split_table_rows)
from .parquet_io import has_pq_vector_index, load_scalar_column, read_index_from_parquet, row_mask_from_expression
from .predicate import allowed, col
from ._ffi import (PQV_L2SQ_REF4, PQV_L2SQ_SEQ, PQV_COSINE, PQV_L2SQ_MFMA, PQV_DOT, PQV_LAYOUT_IVF_ORDERED, PQV_LAYOUT_ROW_ORDER,
                   PQV_RELEASE_ROW_ORDER, PQV_RELEASE_IF_COPIED, PQV_TABLE_CAP_ROUND_ROBIN, PQV_PREPARE_COSINE, PQV_KEY_EQ, PQV_KEY_RANGE, PQV_KEY_IN,
                   PQV_KEY_SET_MAX, LIB_PATH)

__all__ = ["RowMask", "RowKeys", "KeyPartition", "DistinctSearchResult", "GroupSearchResult", "TableDistinctSearchResult", "Column", "col", "allowed", "load_scalar_column", "row_mask_from_expression", "CandidateCursor", "Corpus", "Index", "IndexBuilder", "PqvError", "RangeBuilder", "Searcher", "SearchResult",
           "TopkBuilder", "TableRangeBuilder", "TableSearcher", "TableSearchResult", "TableTopkBuilder", "searcher_for_parquet_files",
           "split_table_rows", "device_count", "merge_topk", "rerank_batch", "rerank_finish", "searcher_for_parquet", "PQV_COSINE", "PQV_L2SQ_MFMA", "PQV_DOT",
           "has_pq_vector_index", "read_index_from_parquet", "PQV_L2SQ_REF4",
           "PQV_L2SQ_SEQ", "PQV_LAYOUT_IVF_ORDERED", "PQV_LAYOUT_ROW_ORDER",
           "PQV_RELEASE_ROW_ORDER", "PQV_RELEASE_IF_COPIED", "PQV_TABLE_CAP_ROUND_ROBIN", "PQV_PREPARE_COSINE", "round_robin_quota", "LIB_PATH",
           "PQV_KEY_EQ", "PQV_KEY_RANGE", "PQV_KEY_IN", "PQV_KEY_SET_MAX"]
