// pqv.hpp -- C++ host-side mirror of the reference's Rust API over the C ABI (include/pqv.h):
//   pqv::IndexBuilder   src/ivf/parquet.rs:23-103   (n_clusters / max_iters / seed builder)
//   pqv::TopkBuilder    src/ivf/search.rs:49-81     (k and nprobe must be set and > 0)
//   pqv::SearchResult   src/ivf/search.rs:41-45
// Header-only RAII wrappers; errors become pqv::Error carrying the reference's message text.
#pragma once
#include <algorithm>
#include <cstdint>
#include <limits>
#include <memory>
#include <optional>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../include/pqv.h"

namespace pqv {

struct Error : std::runtime_error {
    int code;
    Error(int c, const std::string &m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) { if (rc != PQV_OK) throw Error(rc, pqv_last_error()); }

struct SearchResult { uint32_t row_idx; float distance; };

class Corpus {
public:
    Corpus(int device, const float *rows, uint64_t n, uint32_t dim) {
        pqv_corpus *h = nullptr;
        check(pqv_corpus_upload(device, rows, n, dim, &h));
        h_.reset(h);
    }
    pqv_corpus *get() const { return h_.get(); }
    uint64_t rows() const { return pqv_corpus_rows(h_.get()); }
    uint32_t dim() const { return pqv_corpus_dim(h_.get()); }
private:
    struct Del { void operator()(pqv_corpus *p) const { pqv_corpus_free(p); } };
    std::unique_ptr<pqv_corpus, Del> h_;
};

class Index {
public:
    explicit Index(pqv_index *h) : h_(h) {}
    static Index from_bytes(const std::vector<uint8_t> &blob) {
        pqv_index *h = nullptr;
        check(pqv_index_from_bytes(blob.data(), blob.size(), &h));
        return Index(h);
    }
    std::vector<uint8_t> to_bytes() const {
        uint8_t *buf = nullptr; size_t len = 0;
        check(pqv_index_to_bytes(h_.get(), &buf, &len));
        std::vector<uint8_t> out(buf, buf + len);
        pqv_bytes_free(buf);
        return out;
    }
    uint32_t dim() const { return pqv_index_dim(h_.get()); }
    uint32_t n_clusters() const { return pqv_index_n_clusters(h_.get()); }
    pqv_index *get() const { return h_.get(); }
private:
    struct Del { void operator()(pqv_index *p) const { pqv_index_free(p); } };
    std::unique_ptr<pqv_index, Del> h_;
};

class IndexBuilder {
public:
    explicit IndexBuilder(const Corpus &corpus) : corpus_(corpus) {}
    IndexBuilder &n_clusters(uint32_t v) { n_clusters_ = v; return *this; }
    IndexBuilder &max_iters(uint32_t v) { max_iters_ = v; return *this; }
    IndexBuilder &seed(uint64_t v) { seed_ = v; return *this; }
    IndexBuilder &workers(uint32_t v) { workers_ = v; return *this; }
    Index build() const {
        if (max_iters_ == 0) throw Error(PQV_ERR_INVALID, "max_iters must be > 0");      // parquet.rs:90
        if (n_clusters_ && *n_clusters_ == 0) throw Error(PQV_ERR_INVALID, "n_clusters must be > 0"); // :93
        pqv_index *h = nullptr;
        check(pqv_index_build(corpus_.get(), n_clusters_.value_or(0), max_iters_, seed_, workers_, &h));
        return Index(h);
    }
private:
    const Corpus &corpus_;
    std::optional<uint32_t> n_clusters_;
    uint32_t max_iters_ = 20;      // parquet.rs:37
    uint64_t seed_ = 42;           // parquet.rs:38
    uint32_t workers_ = 0;
};

class Searcher {
public:
    Searcher(const Index &index, Corpus &corpus, uint32_t flags = PQV_LAYOUT_IVF_ORDERED) {
        pqv_searcher *h = nullptr;
        check(pqv_searcher_create(index.get(), corpus.get(), flags, &h));
        h_.reset(h);
        dim_ = index.dim();
    }
    pqv_searcher *get() const { return h_.get(); }
    uint32_t dim() const { return dim_; }
    // exact top-k among the rows the caller names per query -- query q's candidates are cand_rows[lims[q] .. lims[q + 1]) in any
    // order, lims [nq + 1]; rows that are not indexed are skipped -- and, with `mask` (a RowMask's get()), that the mask allows
    // (pqv.h: pqv_topk_rows); found[q] results per query, k slots each
    void topk_rows(const std::vector<uint64_t> &lims, const std::vector<uint32_t> &cand_rows, const std::vector<float> &queries, uint32_t k,
                   std::vector<uint32_t> &rows, std::vector<float> &dist, std::vector<uint32_t> &found,
                   const pqv_row_mask *mask = nullptr) const {
        const uint32_t nq = lims.empty() ? 0 : static_cast<uint32_t>(lims.size() - 1);
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, std::numeric_limits<float>::infinity());
        found.assign(nq, 0);
        check(pqv_topk_rows(h_.get(), lims.data(), cand_rows.data(), mask, queries.data(), nq, dim_, k, PQV_L2SQ_REF4, 1, rows.data(),
                            dist.data(), found.data(), nullptr));
    }
    // ... and every candidate's exact distance instead: dist[i - lims[0]] for candidate i, +inf where it is not considered (pqv.h:
    // pqv_score_rows)
    void score_rows(const std::vector<uint64_t> &lims, const std::vector<uint32_t> &cand_rows, const std::vector<float> &queries,
                    std::vector<float> &dist, const pqv_row_mask *mask = nullptr) const {
        const uint32_t nq = lims.empty() ? 0 : static_cast<uint32_t>(lims.size() - 1);
        dist.assign(nq && lims[nq] > lims[0] ? static_cast<size_t>(lims[nq] - lims[0]) : 0, std::numeric_limits<float>::infinity());
        check(pqv_score_rows(h_.get(), lims.data(), cand_rows.data(), mask, queries.data(), nq, dim_, PQV_L2SQ_REF4, 1, dist.data()));
    }
    // MMR top-k: the fetch_k nearest rows of the probed lists (under `mask` where one is given), then k of them picked by maximal
    // marginal relevance with weight lambda on the distance to the query; rows / dist / score in pick order, found[q] picks per
    // query, k slots each (pqv.h: pqv_topk_mmr)
    void topk_mmr(const std::vector<float> &queries, uint32_t k, uint32_t fetch_k, float lambda, uint32_t nprobe, std::vector<uint32_t> &rows,
                  std::vector<float> &dist, std::vector<float> &score, std::vector<uint32_t> &found, const pqv_row_mask *mask = nullptr) const {
        const uint32_t nq = dim_ ? static_cast<uint32_t>(queries.size() / dim_) : 0;
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, std::numeric_limits<float>::infinity());
        score.assign(static_cast<size_t>(nq) * k, std::numeric_limits<float>::infinity());
        found.assign(nq, 0);
        check(pqv_topk_mmr(h_.get(), mask, queries.data(), nq, dim_, k, fetch_k, lambda, nprobe, 0, PQV_L2SQ_REF4, 1, rows.data(), dist.data(),
                           score.data(), found.data(), nullptr));
    }
    // ... and the selection alone over the [nq, n] rows and distances of any top-k call (pqv.h: pqv_mmr_select)
    void mmr_select(const std::vector<uint32_t> &cand_rows, const std::vector<float> &cand_dist, uint32_t nq, uint32_t k, float lambda,
                    std::vector<uint32_t> &rows, std::vector<float> &dist, std::vector<float> &score, std::vector<uint32_t> &found) const {
        const uint32_t n = nq ? static_cast<uint32_t>(cand_rows.size() / nq) : 0;
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, std::numeric_limits<float>::infinity());
        score.assign(static_cast<size_t>(nq) * k, std::numeric_limits<float>::infinity());
        found.assign(nq, 0);
        check(pqv_mmr_select(h_.get(), cand_rows.data(), cand_dist.data(), nullptr, nq, n, k, lambda, PQV_L2SQ_REF4, 1, rows.data(), dist.data(),
                             score.data(), found.data()));
    }
private:
    struct Del { void operator()(pqv_searcher *p) const { pqv_searcher_free(p); } };
    std::unique_ptr<pqv_searcher, Del> h_;
    uint32_t dim_ = 0;
};

// A scalar column resident on one GPU beside the embedding column (pqv.h: pqv_column): what predicate leaves read.
class Column {
public:
    // dtype: PQV_COL_*; values: one per corpus row; valid: empty, or one byte per row (0 = NULL)
    Column(int device, int dtype, const void *values, const std::vector<uint8_t> &valid, uint64_t n_rows) {
        if (!valid.empty() && valid.size() != n_rows) throw Error(PQV_ERR_INVALID, "one validity byte per value");
        pqv_column *h = nullptr;
        check(pqv_column_upload(device, dtype, values, valid.empty() ? nullptr : valid.data(), n_rows, &h));
        h_.reset(h);
    }
    const pqv_column *get() const { return h_.get(); }
    uint64_t rows() const { return pqv_column_rows(h_.get()); }
    int dtype() const { return pqv_column_dtype(h_.get()); }
private:
    struct Del { void operator()(pqv_column *p) const { pqv_column_free(p); } };
    std::unique_ptr<pqv_column, Del> h_;
};

// One allow bit per row of a searcher's corpus (pqv.h: pqv_row_mask); may outlive its searcher or be released before it.
class RowMask {
public:
    // the mask of a predicate evaluated on the GPU (pqv.h: pqv_row_mask_from_predicates): leaf i is (columns[i], ops[i],
    // operands[2 i], operands[2 i + 1]), masks[i] instead of a column for a PQV_OP_MASK leaf (masks may be empty without one)
    static RowMask from_predicates(const Searcher &s, const std::vector<const pqv_column *> &columns,
                                   const std::vector<const pqv_row_mask *> &masks, const std::vector<uint32_t> &ops,
                                   const std::vector<uint64_t> &operands, const std::vector<uint8_t> &program) {
        if (columns.size() != ops.size() || operands.size() != 2 * ops.size() || (!masks.empty() && masks.size() != ops.size()))
            throw Error(PQV_ERR_INVALID, "one column slot and two operands per leaf");
        pqv_row_mask *h = nullptr;
        check(pqv_row_mask_from_predicates(s.get(), static_cast<uint32_t>(ops.size()), columns.data(), masks.empty() ? nullptr : masks.data(),
                                           ops.data(), operands.data(), program.data(), static_cast<uint32_t>(program.size()), nullptr, &h));
        RowMask m;
        m.h_.reset(h);
        return m;
    }
    std::vector<uint8_t> to_bytes() const {
        std::vector<uint8_t> out(rows());
        check(pqv_row_mask_to_bytes(h_.get(), out.data(), out.size()));
        return out;
    }
    RowMask(const Searcher &s, const std::vector<uint8_t> &allowed) {
        pqv_row_mask *h = nullptr;
        check(pqv_row_mask_create(s.get(), allowed.data(), allowed.size(), &h));
        h_.reset(h);
    }
    const pqv_row_mask *get() const { return h_.get(); }
    uint64_t rows() const { return pqv_row_mask_rows(h_.get()); }
    uint64_t count() const { return pqv_row_mask_count(h_.get()); }
private:
    RowMask() = default;
    struct Del { void operator()(pqv_row_mask *p) const { pqv_row_mask_free(p); } };
    std::unique_ptr<pqv_row_mask, Del> h_;
};

// A per-query filter on a key column (pqv.h: pqv_key_filter): equals(keys), between(lo, hi) -- both ends inclusive -- or in_sets(sets),
// one entry per query.  It owns copies of its arrays, a set filter sorts and de-duplicates every set; descriptor() stays valid
// as long as the filter does.
class KeyFilter {
public:
    static KeyFilter equals(std::vector<int64_t> keys) {
        KeyFilter f; f.kind_ = PQV_KEY_EQ; f.a_ = std::move(keys); return f;
    }
    static KeyFilter between(std::vector<int64_t> lo, std::vector<int64_t> hi) {
        if (lo.size() != hi.size()) throw std::invalid_argument("one lower and one upper bound per query");
        KeyFilter f; f.kind_ = PQV_KEY_RANGE; f.a_ = std::move(lo); f.b_ = std::move(hi); return f;
    }
    static KeyFilter in_sets(const std::vector<std::vector<int64_t>> &sets) {
        KeyFilter f; f.kind_ = PQV_KEY_IN; f.lims_.assign(1, 0);
        for (std::vector<int64_t> s : sets) {
            std::sort(s.begin(), s.end());
            s.erase(std::unique(s.begin(), s.end()), s.end());
            if (s.size() > PQV_KEY_SET_MAX) throw std::invalid_argument("a query key set takes at most 1024 values");
            f.b_.insert(f.b_.end(), s.begin(), s.end());
            f.lims_.push_back(f.b_.size());
        }
        if (f.b_.empty()) f.b_.push_back(0);      // (never read: a readable address for the descriptor)
        return f;
    }
    uint32_t queries() const { return static_cast<uint32_t>(kind_ == PQV_KEY_IN ? lims_.size() - 1 : a_.size()); }
    pqv_key_filter descriptor() const {
        return pqv_key_filter{kind_, 0, kind_ == PQV_KEY_IN ? static_cast<const void *>(lims_.data()) : static_cast<const void *>(a_.data()),
                              kind_ == PQV_KEY_EQ ? nullptr : static_cast<const void *>(b_.data())};
    }
private:
    KeyFilter() = default;
    uint32_t kind_ = PQV_KEY_EQ;
    std::vector<int64_t> a_, b_;
    std::vector<uint64_t> lims_;
};

// A key column laid out for one searcher (pqv.h: pqv_row_keys): every query of a keyed call is filtered by ITS OWN
// `column == key`.  The column is copied; keys may outlive their searcher or be released before it.
class RowKeys {
public:
    RowKeys(const Searcher &s, const Column &column) {
        pqv_row_keys *h = nullptr;
        check(pqv_row_keys_create(s.get(), column.get(), nullptr, &h));
        h_.reset(h);
    }
    const pqv_row_keys *get() const { return h_.get(); }
    uint64_t rows() const { return pqv_row_keys_rows(h_.get()); }
    int dtype() const { return pqv_row_keys_dtype(h_.get()); }
    // top-k of nq = qkeys.size() queries (queries: [nq, dim]), query q over the rows whose key equals qkeys[q] -- and, with `mask`,
    // that the mask allows (pqv.h: pqv_topk_keyed); found[q] results per query, k slots each
    void topk(const Searcher &s, const std::vector<int64_t> &qkeys, const std::vector<float> &queries, uint32_t k, uint32_t nprobe,
              std::vector<uint32_t> &rows, std::vector<float> &dist, std::vector<uint32_t> &found, const RowMask *mask = nullptr) const {
        const uint32_t nq = static_cast<uint32_t>(qkeys.size());
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, 0.0f);
        found.assign(nq, 0);
        check(pqv_topk_keyed(s.get(), h_.get(), qkeys.data(), mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, nprobe, 0,
                             PQV_L2SQ_REF4, 1, rows.data(), dist.data(), found.data(), nullptr));
    }
    // the same under any per-query filter -- a key, a range, a set (pqv.h: pqv_topk_filtered); nq = filter.queries()
    void topk(const Searcher &s, const KeyFilter &filter, const std::vector<float> &queries, uint32_t k, uint32_t nprobe,
              std::vector<uint32_t> &rows, std::vector<float> &dist, std::vector<uint32_t> &found, const RowMask *mask = nullptr) const {
        const uint32_t nq = filter.queries();
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, 0.0f);
        found.assign(nq, 0);
        const pqv_key_filter d = filter.descriptor();
        check(pqv_topk_filtered(s.get(), h_.get(), &d, mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, nprobe, 0,
                                PQV_L2SQ_REF4, 1, rows.data(), dist.data(), found.data(), nullptr));
    }
    // distinct top-k with this column as the GROUP column (pqv.h: pqv_topk_distinct): per query the nearest row of each of the k
    // nearest key values; found[q] groups per query, k slots each, group_keys the representatives' key values
    void topk_distinct(const Searcher &s, const std::vector<float> &queries, uint32_t k, uint32_t nprobe, std::vector<uint32_t> &rows,
                       std::vector<float> &dist, std::vector<int64_t> &group_keys, std::vector<uint32_t> &found,
                       const RowMask *mask = nullptr) const {
        const uint32_t nq = s.dim() ? static_cast<uint32_t>(queries.size() / s.dim()) : 0;
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, 0.0f);
        group_keys.assign(static_cast<size_t>(nq) * k, 0);
        found.assign(nq, 0);
        check(pqv_topk_distinct(s.get(), h_.get(), mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, nprobe, 0, PQV_L2SQ_REF4, 1,
                                rows.data(), dist.data(), group_keys.data(), found.data(), nullptr));
    }
    // grouped top-k (pqv.h: pqv_topk_grouped): up to group_size rows of each of the k nearest key values; rows / dist are [nq, k,
    // group_size], group_keys / group_rows [nq, k] (the rows returned per group), found[q] groups per query
    void topk_grouped(const Searcher &s, const std::vector<float> &queries, uint32_t k, uint32_t group_size, uint32_t nprobe,
                      std::vector<uint32_t> &rows, std::vector<float> &dist, std::vector<int64_t> &group_keys,
                      std::vector<uint32_t> &group_rows, std::vector<uint32_t> &found, const RowMask *mask = nullptr) const {
        const uint32_t nq = s.dim() ? static_cast<uint32_t>(queries.size() / s.dim()) : 0;
        rows.assign(static_cast<size_t>(nq) * k * group_size, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k * group_size, std::numeric_limits<float>::infinity());
        group_keys.assign(static_cast<size_t>(nq) * k, 0);
        group_rows.assign(static_cast<size_t>(nq) * k, 0);
        found.assign(nq, 0);
        check(pqv_topk_grouped(s.get(), h_.get(), mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, group_size, nprobe, 0,
                               PQV_L2SQ_REF4, 1, rows.data(), dist.data(), group_keys.data(), group_rows.data(), found.data(), nullptr));
    }
    // topk_distinct / topk_grouped with one filter PER QUERY on `filter_keys` (it may be this column), applied before a group's
    // representative is chosen (pqv.h: pqv_topk_distinct_filtered, pqv_topk_grouped_filtered); nq = filter.queries()
    void topk_distinct_filtered(const Searcher &s, const RowKeys &filter_keys, const KeyFilter &filter, const std::vector<float> &queries,
                                uint32_t k, uint32_t nprobe, std::vector<uint32_t> &rows, std::vector<float> &dist,
                                std::vector<int64_t> &group_keys, std::vector<uint32_t> &found, const RowMask *mask = nullptr) const {
        const uint32_t nq = filter.queries();
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, 0.0f);
        group_keys.assign(static_cast<size_t>(nq) * k, 0);
        found.assign(nq, 0);
        const pqv_key_filter d = filter.descriptor();
        check(pqv_topk_distinct_filtered(s.get(), h_.get(), filter_keys.get(), &d, mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k,
                                         nprobe, 0, PQV_L2SQ_REF4, 1, rows.data(), dist.data(), group_keys.data(), found.data(), nullptr));
    }
    void topk_grouped_filtered(const Searcher &s, const RowKeys &filter_keys, const KeyFilter &filter, const std::vector<float> &queries,
                               uint32_t k, uint32_t group_size, uint32_t nprobe, std::vector<uint32_t> &rows, std::vector<float> &dist,
                               std::vector<int64_t> &group_keys, std::vector<uint32_t> &group_rows, std::vector<uint32_t> &found,
                               const RowMask *mask = nullptr) const {
        const uint32_t nq = filter.queries();
        rows.assign(static_cast<size_t>(nq) * k * group_size, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k * group_size, std::numeric_limits<float>::infinity());
        group_keys.assign(static_cast<size_t>(nq) * k, 0);
        group_rows.assign(static_cast<size_t>(nq) * k, 0);
        found.assign(nq, 0);
        const pqv_key_filter d = filter.descriptor();
        check(pqv_topk_grouped_filtered(s.get(), h_.get(), filter_keys.get(), &d, mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k,
                                        group_size, nprobe, 0, PQV_L2SQ_REF4, 1, rows.data(), dist.data(), group_keys.data(), group_rows.data(),
                                        found.data(), nullptr));
    }
    // topk_distinct / topk_grouped probing on until k GROUPS are found (pqv.h: pqv_topk_distinct_expand, pqv_topk_grouped_expand): every
    // query walks the fewest lists in [nprobe, max_nprobe] that hold k distinct values of this column; used[q] = that many.
    // filter_keys / filter: both or neither (nullptr: the unfiltered twins)
    void topk_distinct_expand(const Searcher &s, const RowKeys *filter_keys, const KeyFilter *filter, const std::vector<float> &queries,
                              uint32_t k, uint32_t nprobe, uint32_t max_nprobe, std::vector<uint32_t> &rows, std::vector<float> &dist,
                              std::vector<int64_t> &group_keys, std::vector<uint32_t> &found, std::vector<uint32_t> &used,
                              const RowMask *mask = nullptr) const {
        const uint32_t nq = s.dim() ? static_cast<uint32_t>(queries.size() / s.dim()) : 0;
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, 0.0f);
        group_keys.assign(static_cast<size_t>(nq) * k, 0);
        found.assign(nq, 0);
        used.assign(nq, 0);
        pqv_key_filter d{};
        if (filter) d = filter->descriptor();
        check(pqv_topk_distinct_expand(s.get(), h_.get(), filter_keys ? filter_keys->get() : nullptr, filter ? &d : nullptr,
                                       mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, nprobe, max_nprobe, PQV_L2SQ_REF4, 1,
                                       rows.data(), dist.data(), group_keys.data(), found.data(), nullptr, used.data()));
    }
    void topk_grouped_expand(const Searcher &s, const RowKeys *filter_keys, const KeyFilter *filter, const std::vector<float> &queries,
                             uint32_t k, uint32_t group_size, uint32_t nprobe, uint32_t max_nprobe, std::vector<uint32_t> &rows,
                             std::vector<float> &dist, std::vector<int64_t> &group_keys, std::vector<uint32_t> &group_rows,
                             std::vector<uint32_t> &found, std::vector<uint32_t> &used, const RowMask *mask = nullptr) const {
        const uint32_t nq = s.dim() ? static_cast<uint32_t>(queries.size() / s.dim()) : 0;
        rows.assign(static_cast<size_t>(nq) * k * group_size, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k * group_size, std::numeric_limits<float>::infinity());
        group_keys.assign(static_cast<size_t>(nq) * k, 0);
        group_rows.assign(static_cast<size_t>(nq) * k, 0);
        found.assign(nq, 0);
        used.assign(nq, 0);
        pqv_key_filter d{};
        if (filter) d = filter->descriptor();
        check(pqv_topk_grouped_expand(s.get(), h_.get(), filter_keys ? filter_keys->get() : nullptr, filter ? &d : nullptr,
                                      mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, group_size, nprobe, max_nprobe,
                                      PQV_L2SQ_REF4, 1, rows.data(), dist.data(), group_keys.data(), group_rows.data(), found.data(), nullptr,
                                      used.data()));
    }
private:
    struct Del { void operator()(pqv_row_keys *p) const { pqv_row_keys_free(p); } };
    std::unique_ptr<pqv_row_keys, Del> h_;
};

// A posting list per key value over one searcher's rows (pqv.h: pqv_key_partition): the exact top-k over a key's own rows, nothing
// probed.  The column is read once; a partition may outlive its searcher or be released before it.
class KeyPartition {
public:
    KeyPartition(const Searcher &s, const Column &column) {
        pqv_key_partition *h = nullptr;
        check(pqv_key_partition_create(s.get(), column.get(), nullptr, &h));
        h_.reset(h);
    }
    const pqv_key_partition *get() const { return h_.get(); }
    uint64_t rows() const { return pqv_key_partition_rows(h_.get()); }
    uint64_t n_keys() const { return pqv_key_partition_n_keys(h_.get()); }
    int dtype() const { return pqv_key_partition_dtype(h_.get()); }
    // the distinct key values ascending and their row counts
    void keys(std::vector<int64_t> &values, std::vector<uint64_t> &counts) const {
        values.assign(n_keys(), 0);
        counts.assign(n_keys(), 0);
        check(pqv_key_partition_keys(h_.get(), values.data(), counts.data(), values.size()));
    }
    // exact top-k of nq = filter.queries() queries over the partition rows whose key passes the query's filter -- and, with `mask`,
    // that the mask allows (pqv.h: pqv_topk_partition); found[q] results per query, k slots each
    void topk(const Searcher &s, const KeyFilter &filter, const std::vector<float> &queries, uint32_t k, std::vector<uint32_t> &rows,
              std::vector<float> &dist, std::vector<uint32_t> &found, const RowMask *mask = nullptr) const {
        const uint32_t nq = filter.queries();
        rows.assign(static_cast<size_t>(nq) * k, 0xFFFFFFFFu);
        dist.assign(static_cast<size_t>(nq) * k, 0.0f);
        found.assign(nq, 0);
        const pqv_key_filter d = filter.descriptor();
        check(pqv_topk_partition(s.get(), h_.get(), &d, mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), k, PQV_L2SQ_REF4, 1,
                                 rows.data(), dist.data(), found.data(), nullptr));
    }
    // every partition row whose key passes the query's filter within `radius` of the query -- and, with `mask`, that the mask allows
    // (pqv.h: pqv_range_search_partition): exact, ascending by (distance, sequence position); query q's hits are rows / dist
    // [lims[q], lims[q + 1]); max_results > 0 keeps the first max_results of each query
    void range_search(const Searcher &s, const KeyFilter &filter, const std::vector<float> &queries, float radius, std::vector<uint64_t> &lims,
                      std::vector<uint32_t> &rows, std::vector<float> &dist, const RowMask *mask = nullptr, uint64_t max_results = 0) const {
        const uint32_t nq = filter.queries();
        const pqv_key_filter d = filter.descriptor();
        uint64_t *l = nullptr;
        uint32_t *r = nullptr;
        float *x = nullptr;
        check(pqv_range_search_partition(s.get(), h_.get(), &d, mask ? mask->get() : nullptr, queries.data(), nq, s.dim(), radius, max_results,
                                         PQV_L2SQ_REF4, 1, &l, &r, &x, nullptr, nullptr));
        lims.assign(l, l + nq + 1);
        rows.assign(r, r + lims[nq]);
        dist.assign(x, x + lims[nq]);
        pqv_range_free(l, r, x);
    }
private:
    struct Del { void operator()(pqv_key_partition *p) const { pqv_key_partition_free(p); } };
    std::unique_ptr<pqv_key_partition, Del> h_;
};

class TopkBuilder {
public:
    TopkBuilder(const Searcher &s, const std::vector<float> &query) : s_(s), query_(query) {}
    // only rows the mask allows are considered (the reference's predicate inside the scan, exec.rs:207-277)
    TopkBuilder &where(const RowMask &m) { mask_ = &m; return *this; }
    TopkBuilder &k(uint32_t v) { if (!v) throw Error(PQV_ERR_INVALID, "k must be > 0"); k_ = v; return *this; }
    TopkBuilder &nprobe(uint32_t v) { if (!v) throw Error(PQV_ERR_INVALID, "nprobe must be > 0"); nprobe_ = v; return *this; }
    // PQV_L2SQ_REF4 (default: sqrt(d2) as the reference returns it), PQV_COSINE (0.5 d2 of the normalised vectors) or PQV_DOT
    // (-(q.x), smallest first); see include/pqv.h
    TopkBuilder &metric(int m) {
        if (m != PQV_L2SQ_REF4 && m != PQV_COSINE && m != PQV_DOT) throw Error(PQV_ERR_INVALID, "unknown metric");
        metric_ = m; return *this;
    }
    std::vector<SearchResult> search() const {
        if (!k_) throw Error(PQV_ERR_INVALID, "k must be set");              // search.rs:77
        if (!nprobe_) throw Error(PQV_ERR_INVALID, "nprobe must be set");    // search.rs:78
        std::vector<uint32_t> rows(*k_);
        std::vector<float> dist(*k_);
        uint32_t found = 0;
        if (mask_)
            check(pqv_topk_masked(s_.get(), mask_->get(), query_.data(), 1, static_cast<uint32_t>(query_.size()), *k_, *nprobe_, 0,
                                  metric_, 1, rows.data(), dist.data(), &found, nullptr));
        else
        check(pqv_topk(s_.get(), query_.data(), 1, static_cast<uint32_t>(query_.size()), *k_, *nprobe_, 0,
                       metric_, 1, rows.data(), dist.data(), &found, nullptr));
        std::vector<SearchResult> out;
        for (uint32_t i = 0; i < found; ++i) out.push_back({rows[i], dist[i]});
        return out;
    }
private:
    const Searcher &s_;
    const std::vector<float> &query_;
    std::optional<uint32_t> k_, nprobe_;
    int metric_ = PQV_L2SQ_REF4;
    const RowMask *mask_ = nullptr;
};

}  // namespace pqv
