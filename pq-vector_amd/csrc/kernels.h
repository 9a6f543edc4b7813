// kernels.h -- host-callable launchers of the gfx950 kernels (internal; the public
// boundary is include/pqv.h).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace pqv {

// Sentinel key: sorts after every real (d2, position) key.
constexpr uint64_t KEY_EMPTY = ~0ull;

// What a streaming distance pass does with each row's exact d2.
enum StreamMode : int {
    STREAM_TOPK   = 0,  // fold into per-wave top-k lists
    STREAM_DIST   = 1,  // out_f32[pos] = d2
    STREAM_MINUPD = 2,  // out_f32[pos] = min(out_f32[pos], d2)   (k-means++ round)
    STREAM_RANGE  = 3,  // out <= radius: append (d2, pos) key + storage row to the query's hit segment (range search)
};

struct StreamArgs {
    // row storage [*, dim] f32; a list position p maps to storage row (row_of ? row_of[p] : p)
    const float    *mat;
    const uint32_t *row_of;
    // inverted-list offsets in list positions; probe == nullptr => a single list
    // [single_begin, single_end) is scanned for every query
    const uint64_t *list_off;
    const uint32_t *probe;       // [nq, nprobe] cluster ids in probe-rank order
    const uint64_t *cand_base;   // [nq, nprobe] candidate position of each probed list's first row
    uint64_t        single_begin, single_end;
    const float    *queries;     // [nq, dim]
    uint32_t        nq, nprobe, dim, k;
    uint32_t        rows_per_block;   // multiple of 256
    uint32_t        blocks_per_list;  // gridDim.x
    uint64_t        max_pos;          // candidates at position >= max_pos are ignored
    const uint64_t *pair_end;         // [nq, nprobe] or nullptr: list j of query q counts positions < pair_end[q * nprobe + j]
                                      // instead (a round-robin capped table, SegProbeArgs::pair_end)
    int             metric;           // pqv_metric
    // TOPK outputs: [nq][nprobe*blocks_per_list*4][k]
    uint64_t       *part_keys;
    uint32_t       *part_vals;
    // DIST / MINUPD output, indexed by candidate position (single-list mode)
    float          *out_f32;
    // MINUPD, optional: every value this pass writes to out_f32 is also written here (pinned host memory that starts as a
    // copy of out_f32: the k-means++ host scan reads it after the stream is drained, with no copy command between the
    // rounds' kernels, and only the minima that changed cross the bus)
    float          *mirror_f32;
    // MINUPD, optional second mirror in CHUNK-TRANSPOSED order: entry pos goes to mirror_t[(pos % mirror_chunk) * mirror_stride +
    // pos / mirror_chunk], so the host adds the w chunk chains of index.rs:356-370 with vector instructions (lane = chunk)
    float          *mirror_t;
    uint32_t        mirror_chunk, mirror_stride;
    // optional: zero_u32[0 .. zero_n) = 0 (scratch of the kernels that follow in the stream)
    uint32_t       *zero_u32;
    uint32_t        zero_n;
    // RANGE: probe ranks [j0, j0 + nj) of every query (gridDim.y = nj; probe / cand_base keep the row stride nprobe).  A
    // candidate is a hit iff out = (sqrt_out 1 ? sqrt(d2) : 2 ? 0.5 d2 (PQV_COSINE) : d2) <= radius; each wave appends its hits to query q's segment
    // hit_keys / hit_vals [q * seg_stride + slot) (slot from one atomicAdd per wave on hit_cnt[q]).  seg_stride must be at
    // least the query's capped candidate count, so a segment cannot overflow.
    uint32_t        j0, nj;
    float           radius;
    int             sqrt_out;
    uint32_t       *hit_cnt;     // [nq], zeroed by the caller
    uint64_t       *hit_keys;    // (d2 bits << 32) | candidate position
    uint32_t       *hit_vals;    // storage row
    uint64_t        seg_stride;
    // optional [nq]: PACKED segments -- query q's begins at seg_off[q] instead of q * seg_stride (range_seg_base; the partition
    // range search, whose segment lengths are its per-query candidate counts).  nullptr: the uniform stride.
    const uint64_t *seg_off;
};
// the first entry of query q's hit segment, for the kernel that appends (emit_range_hit) and the ones that sort and write out
__host__ __device__ __forceinline__ uint64_t range_seg_base(const uint64_t *seg_off, uint64_t seg_stride, uint32_t q) {
    return seg_off ? seg_off[q] : (uint64_t)q * seg_stride;
}

// Streaming exact-order squared-L2 pass (the re-rank kernel).  Returns hipError_t.
hipError_t launch_stream(const StreamArgs &a, StreamMode mode, hipStream_t s);

// ---- row-masked searches (kernels_mask.hip) ------------------------------------------------------------------------------
// A row mask on the device is a bitset over LIST POSITIONS: bit p = the caller's allow byte of the row position p reports.
// launch_mask_layout writes it from allow bytes in row order (ids: list position -> reported row, a searcher's d_ids) -- all
// n_words words, n_words >= ceil(n_pos / 64) + 1, bits of positions >= n_pos zero -- and adds the allowed total to *count.
hipError_t launch_mask_layout(const uint8_t *allowed, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos, uint64_t *bits,
                              uint64_t n_words, unsigned long long *count, hipStream_t s);
struct MaskedArgs {
    const uint64_t     *bits;     // the image above
    unsigned long long *stats;    // optional: the searcher's statistics block -- every wave adds the rows it evaluated to the
                                  // embeddings_fetched word of its query's slot (the probe merge of a masked call gets no MergeArgs::stats)
    const uint64_t     *n_cand;   // optional [nq] (with stats): the probe merge's uncapped totals, added to candidate_rows once per query
    const uint32_t     *rank_limit;   // optional [nq] (STREAM_TOPK; pqv_topk_expand): query q walks its probe ranks below rank_limit[q] only -- a
                                      // block of a rank at or beyond it reads that word, stores its four EMPTY lists and ends.  nullptr: every rank
};
// launch_stream's STREAM_TOPK / STREAM_RANGE pass over the allowed positions only (masked_stream_kernel): the same grid, chain
// arithmetic, keys and output formats; a.probe / a.list_off / a.cand_base are required.
hipError_t launch_masked_stream(const StreamArgs &a, const MaskedArgs &ma, StreamMode mode, hipStream_t s);
// the same walk with no mask (bits == nullptr) under MaskedArgs::rank_limit, STREAM_TOPK: the plain call's keys, a cut rank's lists EMPTY
hipError_t launch_limited_stream(const StreamArgs &a, const MaskedArgs &ma, hipStream_t s);

// ---- inner-product search (kernels_dot.hip; pqv.h: PQV_DOT) ----------------------------------------------------------------
// launch_stream's / launch_masked_stream's STREAM_TOPK / STREAM_RANGE pass with dist = 0.0f - s(q, x), s the 4-grouped chain over
// products, and keys (ord(dist) << 32) | candidate position (ord: the order-preserving map of signed f32 bits to u32).  ma ==
// nullptr: every position (a.probe == nullptr: the single list, the centroid probe of a DOT call); else the mask's set positions.
// A hit of STREAM_RANGE: dist <= radius (sqrt_out is not read).  zero_u32 must be unset.
hipError_t launch_dot_stream(const StreamArgs &a, const MaskedArgs *ma, StreamMode mode, hipStream_t s);
struct MergeArgs;
// the fold of those per-wave lists, one wave per query (dot_merge_kernel): part_keys / part_vals / nq / n_part / k_part / k / k_out /
// ids / row_idx / dist / n_found as launch_merge_final reads them; dist = ord undone, tie_flag (where given) written with zeros
hipError_t launch_dot_merge(const MergeArgs &a, hipStream_t s);
// range write-out: dist[i] held ord bits (the range_* kernels with sqrt_out 0), now the distance; i < n
hipError_t launch_dot_finish(float *dist, uint64_t n, hipStream_t s);

// ---- per-query key filters (kernels_mask.hip; pqv.h: pqv_row_keys) ------------------------------------------------------
// A key column on the device is laid out by LIST POSITION like a mask: key_pos[p] = column[ids[p]] at the column's own width
// (elem_size 4 or 8), and -- where the column has validity bytes -- valid_pos, a bitset in exactly the mask image's format.
// launch_key_layout writes all n_words * 64 entries of key_pos (zero behind n_pos: a whole 64-position window behind the last
// position is readable) and, with `valid`, all n_words words of valid_pos; n_words >= ceil(n_pos / 64) + 1.
hipError_t launch_key_layout(const void *values, const uint8_t *valid, uint32_t elem_size, uint64_t n_rows, const uint32_t *ids,
                             uint64_t n_pos, void *key_pos, uint64_t *valid_pos, uint64_t n_words, hipStream_t s);
struct KeyedArgs {
    const uint64_t     *bits;       // optional: a shared row mask's image (MaskedArgs::bits), ANDed into every window
    unsigned long long *stats;      // as MaskedArgs::stats
    const uint64_t     *n_cand;     // as MaskedArgs::n_cand
    const void         *key_pos;    // i32 / i64 [n_words * 64]
    const uint64_t     *valid_pos;  // optional [n_words]
    const int64_t      *qkeys;      // [nq]: query q's key; an i32 column's values are widened for the comparison
    uint32_t            elem_size;  // 4 or 8
    const uint32_t     *rank_limit; // as MaskedArgs::rank_limit
};
// launch_masked_stream with a window's bits taken from key_pos[p] == qkeys[q] (masked_stream_kernel, WIN = 1 / 2)
hipError_t launch_keyed_stream(const StreamArgs &a, const KeyedArgs &ka, StreamMode mode, hipStream_t s);
// A per-query filter descriptor (pqv.h: pqv_key_filter) on the device.  kind 0 (PQV_KEY_EQ): a = qkeys, the call above.  kind 1
// (PQV_KEY_RANGE): a / b = i64 [nq] inclusive bounds, the window is the ballot of a[q] <= key && key <= b[q] (WIN = 3 / 4).  kind 2
// (PQV_KEY_IN): a = u64 lims [nq + 1], b = i64 values; the block copies b[a[q] .. a[q + 1]) -- at most KEY_SET_MAX values of it --
// into LDS and a lane's key is looked up there (WIN = 5 / 6).  KeyedArgs::qkeys is not read for kinds 1 and 2.
constexpr uint32_t KEY_SET_MAX = 1024;
struct KeyFilterArgs : KeyedArgs {
    uint32_t    kind;
    const void *a;
    const void *b;
};
hipError_t launch_key_filter_stream(const StreamArgs &a, const KeyFilterArgs &fa, StreamMode mode, hipStream_t s);

// ---- key partitions (kernels_partition.hip; pqv.h: pqv_key_partition) -----------------------------------------------------
// A key partition on the device: the searcher's list positions whose row has a valid key, sorted by (key as i64, row id) -- pos
// [m] --, the distinct key values ascending -- keys [n_keys] -- and the first entry of every value's run -- key_off [n_keys + 1].
// The build, in the order the host enqueues it (every step on `s`; `tmp` / tmp_bytes: launch_partition_tmp_bytes(n_pos) of scratch):
//   launch_partition_gather    row_key[p] = the row list position p reports where it has a valid key, 0xFFFFFFFF where it has none;
//                              pos[p] = p; *count += the positions with a key (zeroed by the caller)
//   launch_partition_sort_rows (row_key, pos) sorted by row: the m positions with a key come first, in row order
//   launch_partition_keys      key[i] = the column's value of row_key[i], widened, i < m
//   launch_partition_sort_keys (key, pos) sorted STABLY by key as a signed 64-bit value: the (key, row) order
//   launch_partition_runs      the distinct values, each value's run length and *n_keys; then key_off = the lengths' prefix sums
// The two sorts, the run-length pass and the scan are rocPRIM's (header-only, from the ROCm tree; stable LSD radix sorts).
hipError_t launch_partition_tmp_bytes(uint64_t n_pos, size_t *bytes);
hipError_t launch_partition_gather(const uint8_t *valid, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos, uint32_t *row_key, uint32_t *pos,
                                   unsigned long long *count, hipStream_t s);
hipError_t launch_partition_sort_rows(const uint32_t *row_key, const uint32_t *pos, uint32_t *row_key_out, uint32_t *pos_out, uint64_t n_pos,
                                      void *tmp, size_t tmp_bytes, hipStream_t s);
hipError_t launch_partition_keys(const void *values, uint32_t elem_size, const uint32_t *row_key, uint64_t m, int64_t *key, hipStream_t s);
hipError_t launch_partition_sort_keys(const int64_t *key, const uint32_t *pos, int64_t *key_out, uint32_t *pos_out, uint64_t m, void *tmp,
                                      size_t tmp_bytes, hipStream_t s);
// cnt: [m] u64 scratch (the run lengths); key_off[n_keys] = m is written too (key_off has m + 1 entries of room)
hipError_t launch_partition_runs(const int64_t *key, uint64_t m, int64_t *keys, uint64_t *cnt, uint64_t *key_off, unsigned long long *n_keys,
                                 void *tmp, size_t tmp_bytes, hipStream_t s);
// partition_span_kernel: query q's candidate sequence as spans of the partition.  kind 0 (PQV_KEY_EQ, a = i64 [nq]) and 1
// (PQV_KEY_RANGE, a / b = i64 [nq] inclusive bounds): ONE span, span_beg[q] its first entry.  kind 2 (PQV_KEY_IN, a = u64 lims [nq + 1],
// b = i64 values, at most KEY_SET_MAX of a slice are read): a span per slice value, span_beg[q * KEY_SET_MAX + i] and the inclusive
// prefix sums of the span lengths span_end[q * KEY_SET_MAX + i], n_span[q] = the values read.  n_cand[q] (and n_cand_out[q], where
// given) = the sequence's length, saturated at 2^32 - 1 like the prefix sums (a sequence position is a u32); with stats, added to
// candidate_rows.  An empty or inverted range, an absent key and a value no key of the column can take give an empty span.
struct PartitionSpanArgs {
    const int64_t      *keys;       // [n_keys] ascending
    const uint64_t     *key_off;    // [n_keys + 1]
    uint64_t            n_keys;
    uint32_t            nq, kind;
    const void         *a, *b;
    uint32_t           *span_beg;   // [nq] / [nq * KEY_SET_MAX]
    uint32_t           *span_end;   // kind 2: [nq * KEY_SET_MAX]
    uint32_t           *n_span;     // kind 2: [nq]
    uint64_t           *n_cand;     // [nq]
    uint64_t           *n_cand_out; // optional [nq]
    unsigned long long *stats;      // optional: the searcher's statistics block
};
hipError_t launch_partition_span(const PartitionSpanArgs &a, hipStream_t s);
// partition_stream_kernel: launch_masked_stream's STREAM_TOPK pass over a query's candidate sequence instead of probed lists.  grid
// (blocks_per_list = B, nq); wave w of block x takes the 64-position windows (turn * B + x) * 4 + w of its query's sequence, maps
// each sequence position to its partition entry (one span: an add; kind 2: a search in span_end), loads the entry's list position
// and -- with a mask -- keeps the positions whose image bit is set (PartitionSeq::windows / filtered_windows, stream_walk.hpp: the
// one walk of every launch_partition_* pass; partition_walk_ok is what all of them ask of a and pa).  Keys are (distance key << 32) | sequence position, the L2 forms'
// (l2_key) or PQV_DOT's (dot_key); the per-wave lists go out in StreamArgs' format with nprobe = 1.  a.probe / list_off / cand_base
// are not read; a.nprobe must be 1.  Every wave adds the rows it evaluated to embeddings_fetched.
struct PartitionArgs {
    const uint32_t     *pos;        // [m] the partition's list positions
    const uint32_t     *span_beg, *span_end, *n_span;       // launch_partition_span's outputs
    const uint64_t     *n_cand;
    uint32_t            kind;       // the span kernel's
    const uint64_t     *bits;       // optional: a shared row mask's image (MaskedArgs::bits)
    unsigned long long *stats;      // as MaskedArgs::stats
};
hipError_t launch_partition_stream(const StreamArgs &a, const PartitionArgs &pa, hipStream_t s);
// Distinct / grouped top-k over a partition (kernels_partition_group.hip; pqv.h: pqv_topk_partition_grouped): the two passes of
// launch_distinct_stream / launch_grouped_stream over launch_partition_stream's grid and sequence walk, PQV_DOT excepted.  A
// position is walked iff pa.bits allows it AND the group column's valid_pos does (both gathered per list position; either may be
// nullptr); keys are l2_key(sum, sequence position).  Pass 1 (partition_distinct_stream_kernel) writes a.part_keys / a.part_vals /
// da.part_grp [nq][B * 4][k] for launch_distinct_merge with n_part = B * 4.  Pass 2 (partition_grouped_stream_kernel; behind
// launch_group_set) walks the members of the query's set only and writes ga.part_keys / part_vals / part_slot [nq][B * 4][km] and
// ga.part_cnt [nq][B * 4] for launch_grouped_merge.  The mask and the statistics block are pa's: da / ga .bits, .stats, .n_cand
// and .rank_limit are not read.
struct DistinctArgs;
struct GroupedArgs;
hipError_t launch_partition_distinct_stream(const StreamArgs &a, const PartitionArgs &pa, const DistinctArgs &da, hipStream_t s);
hipError_t launch_partition_grouped_stream(const StreamArgs &a, const PartitionArgs &pa, const GroupedArgs &ga, hipStream_t s);
// Range search over a partition (kernels_partition_range.hip; pqv.h: pqv_range_search_partition): launch_partition_stream's grid
// and sequence walk with STREAM_RANGE's output -- every considered row whose output-scale distance is <= a.radius (a.sqrt_out as
// StreamArgs documents it; PQV_DOT: dist <= radius) is appended, as (l2_key / dot_key of the sequence position, storage row), to
// query q's segment of a.hit_keys / a.hit_vals at range_seg_base(a.seg_off, a.seg_stride, q), slot from one atomicAdd per wave and
// tile on a.hit_cnt[q] (zeroed by the caller).  A segment must hold n_cand[q] entries.  a.k / part_keys / part_vals are not read;
// a.nprobe must be 1.  Every wave adds the rows it evaluated to embeddings_fetched.  The segments go to launch_range_sort_*.
hipError_t launch_partition_range(const StreamArgs &a, const PartitionArgs &pa, hipStream_t s);

// ---- candidate lists (kernels_rows.hip; pqv.h: pqv_topk_rows, pqv_score_rows) -----------------------------------------------
// The searcher's row -> list position map: map[r] = the list position that reports row r (ids[p] == r), 0xFFFFFFFF where no list
// holds r; map_len = the corpus' rows, an id at or beyond it is dropped.  A fill and one scatter over the n_pos positions, on `s`.
hipError_t launch_row_map(const uint32_t *ids, uint64_t n_pos, uint32_t *map, uint64_t map_len, hipStream_t s);
// rows_stream_kernel: launch_partition_stream's grid, tile, keys and output format over caller-given sequences -- query q's is
// cand_rows[lims[q] .. lims[q + 1]) as given (at most 2^32 - 1 positions of it; none where the slice is inverted), a position's
// list position map[row] behind a compare of the row against map_len.  A position is walked iff that entry is a list position and
// `bits` allows it; the walk is always the filtered one (walk_seq_windows, stream_walk.hpp).  Block 0 of a query writes
// n_cand_out[q] = the sequence's length and adds it to candidate_rows; every wave adds the rows it evaluated to embeddings_fetched.
struct RowsArgs {
    const uint64_t     *lims;       // [nq + 1] offsets into cand_rows
    const uint32_t     *cand_rows;
    const uint32_t     *map;        // launch_row_map's
    uint64_t            map_len;
    const uint64_t     *bits;       // optional: a shared row mask's image (MaskedArgs::bits)
    unsigned long long *stats;      // as MaskedArgs::stats
    uint64_t           *n_cand_out; // optional [nq]
    const uint64_t     *lims0;      // launch_rows_score: the word the output offsets are taken from (the lims word of the CALL's first
                                    // query, which a piece's lims + q0 no longer begins with)
};
hipError_t launch_rows_stream(const StreamArgs &a, const RowsArgs &ra, hipStream_t s);
// ... with every candidate's distance written instead of offered: a.out_f32[lims[q] - *lims0 + seq] on the output scale (a.sqrt_out
// as StreamArgs documents it; PQV_DOT: 0.0f - s), +inf for a candidate that is not walked.  a.k / part_keys / part_vals are not read.
hipError_t launch_rows_score(const StreamArgs &a, const RowsArgs &ra, hipStream_t s);

// ---- MMR selection (kernels_mmr.hip; pqv.h: pqv_mmr_select, pqv_topk_mmr) ----------------------------------------------------
// mmr_select_kernel, one block per query: the greedy selection of pqv.h's MMR section over query q's candidates cand_rows /
// cand_dist [q * n .. + n), of which the first min(n, n_found_in[q]) whose row the map places in a list are considered.  Of `a` the
// kernel reads mat, row_of, dim, nq, metric (the chain: 1 = SEQ, 4 = PQV_DOT's products) and sqrt_out (how a pairwise d2 is put on
// the output scale, as StreamArgs documents it).  The picks go out in pick order, padded to k with 0xFFFFFFFF / +inf / +inf.
struct MmrArgs {
    const uint32_t *cand_rows;   // [nq, n] row ids, anything
    const float    *cand_dist;   // [nq, n] rel on the output scale
    const uint32_t *n_found_in;  // optional [nq]
    const uint32_t *map;         // launch_row_map's
    uint64_t        map_len;
    uint32_t        n, k;        // n <= 1024, k >= 1
    float           lambda;
    uint32_t       *row_idx;     // [nq, k]
    float          *dist;        // [nq, k]
    float          *score;       // optional [nq, k]
    uint32_t       *n_found;     // optional [nq]
};
hipError_t launch_mmr_select(const StreamArgs &a, const MmrArgs &ma, hipStream_t s);

// ---- expanding filtered top-k (kernels_expand.hip; pqv.h: pqv_topk_expand) ------------------------------------------------
// filter_count_kernel: cnt[q * P + j] = the positions of list probe[q * P + j] that pass the call's filter -- the set bits of
// the windows masked_stream_kernel forms for the same `win` (0: the mask image `bits`; 1 / 2: key_pos == a[q], i32 / i64; 3 / 4:
// a[q] <= key_pos <= b[q]; 5 / 6: key_pos in b[a[q] .. a[q + 1]); valid_pos and a shared mask's bits ANDed in), no candidate cap.
// One block per (rank, query), one plain store each: deterministic.  No embedding is read.
struct ExpandCountArgs {
    const uint32_t *probe;       // [nq, P]
    const uint64_t *list_off;
    uint32_t        nq, P;
    uint32_t        win;         // masked_stream_kernel's WIN
    const uint64_t *bits;        // win 0: the mask's image; else an optional shared mask's
    const void     *key_pos;     // win >= 1
    const uint64_t *valid_pos;   // optional
    const void     *a, *b;       // KeyFilterArgs::a / b (win 1 / 2: a = the query keys)
    uint32_t       *cnt;         // [nq, P]
};
hipError_t launch_filter_count(const ExpandCountArgs &a, hipStream_t s);
// expand_select_kernel, one wave per query: nprobe_used[q] = the smallest p in [p0, P] whose first p lists hold >= k passing
// positions (64-bit prefix sums of cnt in probe order), P where there is none; n_cand[q] is overwritten with the summed length of
// those lists.  1 <= p0 <= P.
struct ExpandSelectArgs {
    const uint32_t *cnt;         // [nq, P]
    const uint32_t *probe;       // [nq, P]
    const uint64_t *cand_base;   // [nq, P]
    const uint64_t *list_off;
    uint32_t        nq, P, p0, k;
    uint32_t       *nprobe_used; // [nq]
    uint64_t       *n_cand;      // [nq]
};
hipError_t launch_expand_select(const ExpandSelectArgs &a, hipStream_t s);
// probe_depth_kernel (pqv.h: pqv_topk_depth), one wave per query behind the probe merge: the raw depth r -- depths[q] (given), or
// the number of ranks j < P whose probe distance d2[q * P + j] is <= the ONE f32 product ratio * d2[q * P] (a NaN on either side
// compares false) -- clamped: nprobe_used[q] = min(max(r, p0), P).  n_cand[q] is overwritten with the summed length of those lists
// and, with `stats`, added to the query's candidate_rows and embeddings_fetched words (the request's probe merge counts nothing).
// pair_end[q * P + j] = ~0 below the depth and 0 from it on: the candidate end of every pair for the kernels that walk by
// (query, rank) -- a cut rank holds no candidate.  1 <= p0 <= P.
struct ProbeDepthArgs {
    const uint32_t *depths;      // [nq] given depths, or nullptr: by ratio
    const uint32_t *d2;          // [nq, P] the probe distances' bits in probe order (MergeArgs::probe_d2); ratio only
    float           ratio;
    const uint32_t *probe;       // [nq, P]
    const uint64_t *cand_base;   // [nq, P]
    const uint64_t *list_off;
    uint32_t        nq, P, p0;
    uint32_t       *nprobe_used; // [nq]
    uint64_t       *n_cand;      // [nq]
    uint64_t       *pair_end;    // [nq, P]
    unsigned long long *stats;   // optional: the searcher's statistics block
    uint32_t       *hist;        // optional (the tile paths' pair sort): the cluster histogram of the pairs BELOW the depths, as the
    uint32_t        hist_stride; // probe merge fills it for a call without depths (MergeArgs::hist: HIST_REPLICAS copies, zeroed)
};
hipError_t launch_probe_depth(const ProbeDepthArgs &a, hipStream_t s);
// the wide screen's seed bounds [nq][P][per_rank] of the ranks at or beyond rank_limit[q] set to +inf ("no bound": the seed kernel
// never visits them, and what an earlier call left there must not be selected) -- for the one-query call, whose selection runs
// inside the seed launch over all P ranks; a batch's selection reads the ranks below the limit only (launch_seed_select)
hipError_t launch_depth_seed_clear(float *seed_ub, const uint32_t *rank_limit, uint32_t nq, uint32_t P, uint32_t per_rank, hipStream_t s);

// ---- expanding distinct / grouped top-k (kernels_group_expand.hip; pqv.h: pqv_topk_distinct_expand) ------------------------
// group_expand_kernel, one block per query: nprobe_used[q] = the smallest p in [p0, P] whose first p lists hold >= k DISTINCT group
// values among the positions the call's stream pass would walk (group validity AND shared mask AND the query's filter, the stream
// kernels' windows from the same pieces), P where there is none; n_cand[q] is overwritten with the summed length of those lists.
// The values are counted exactly in an LDS hash set.  No embedding is read.  1 <= p0 <= P.
constexpr uint32_t GROUP_SET_SLOTS = 4096;         // the set's i64 slots (32 KiB): at most k + 255 <= 1279 are ever filled
constexpr uint64_t GROUP_SET_EMPTY = ~0ull;        // an empty slot; the group value -1 is counted by a flag of its own
// where the set starts to look for (or place) a group value: slot (h + i) % GROUP_SET_SLOTS for i = 0, 1, ... (tests model it)
constexpr uint32_t group_set_home(uint64_t v) { return (uint32_t)((v * 0x9E3779B97F4A7C15ull) >> 52); }
struct GroupFilterArgs;
struct GroupExpandArgs {
    const uint32_t *probe;       // [nq, P]
    const uint64_t *cand_base;   // [nq, P]
    const uint64_t *list_off;
    uint32_t        nq, P, p0, k;
    const uint64_t *bits;        // optional: a shared row mask's image
    const void     *key_pos;     // the group column's position image, i32 / i64
    const uint64_t *valid_pos;   // optional
    uint32_t        elem_size;   // 4 or 8
    uint32_t       *nprobe_used; // [nq]
    uint64_t       *n_cand;      // [nq]
};
// fa == nullptr: no per-query filter
hipError_t launch_group_expand(const GroupExpandArgs &a, const GroupFilterArgs *fa, hipStream_t s);

// ---- distinct top-k (kernels_distinct.hip; pqv.h: pqv_topk_distinct) -----------------------------------------------------
// The group column is a key column's position image (launch_key_layout).  launch_distinct_stream is launch_masked_stream's
// STREAM_TOPK pass over the positions whose key is valid and which the shared mask allows, with per-wave lists that hold at most
// one entry per group value: part_keys / part_vals as there, plus part_grp [nq][nprobe * blocks_per_list * 4][k], the entries'
// group values widened to i64.
struct DistinctArgs {
    const uint64_t     *bits;       // optional: a shared row mask's image (MaskedArgs::bits)
    unsigned long long *stats;      // as MaskedArgs::stats
    const uint64_t     *n_cand;     // as MaskedArgs::n_cand
    const void         *key_pos;    // i32 / i64 [n_words * 64]: the group value of every list position
    const uint64_t     *valid_pos;  // optional [n_words]: positions whose key is not NULL
    uint32_t            elem_size;  // 4 or 8
    int64_t            *part_grp;
    const uint32_t     *rank_limit; // as MaskedArgs::rank_limit (pqv_topk_distinct_expand): the lists of a rank at or beyond it go out EMPTY, group 0
};
hipError_t launch_distinct_stream(const StreamArgs &a, const DistinctArgs &da, hipStream_t s);
// the fold of those lists, one wave per query (distinct_merge_kernel): k <= 1024
struct DistinctMergeArgs {
    const uint64_t *part_keys;   // [nq][n_part][k]
    const uint32_t *part_vals;
    const int64_t  *part_grp;
    uint32_t        nq, n_part, k;
    uint32_t        elem_size;   // the group column's width, 4 or 8 (an i32 column's values are compared in 32 bits)
    const uint32_t *ids;         // storage row -> reported row (nullptr => identity)
    uint32_t       *row_idx;     // [nq, k]
    float          *dist;        // [nq, k]
    int64_t        *group_key;   // [nq, k] or nullptr
    uint32_t       *n_found;     // [nq] or nullptr
    int             sqrt_out;    // 0 d2, 1 sqrt(d2), 2 0.5 d2 (PQV_COSINE)
};
hipError_t launch_distinct_merge(const DistinctMergeArgs &a, hipStream_t s);

// ---- grouped top-k (kernels_grouped.hip; pqv.h: pqv_topk_grouped) --------------------------------------------------------
// Pass 2 of the call: pass 1 (the distinct stream and fold above) has written the k nearest groups' values and n_found.  Every
// launcher takes k * group_size == km <= 1024 with group_size >= 2, hence k <= GROUPED_SET_MAX.
constexpr uint32_t GROUPED_SET_MAX = 512;
// the first n_found[q] values of group_key [nq][k], ascending, to set_keys [nq][k], and each value's rank in pass 1 (its slot) to
// set_slot [nq][k] (group_set_kernel; the padding of group_key is not read)
hipError_t launch_group_set(const int64_t *group_key, const uint32_t *n_found, uint32_t nq, uint32_t k, int64_t *set_keys, uint32_t *set_slot,
                            hipStream_t s);
struct GroupedArgs {
    const uint64_t     *bits;       // optional: a shared row mask's image (MaskedArgs::bits)
    unsigned long long *stats;      // as MaskedArgs::stats: the rows evaluated are added to embeddings_fetched (candidate_rows is pass 1's)
    const void         *key_pos;    // i32 / i64 [n_words * 64]: the group value of every list position
    const uint64_t     *valid_pos;  // optional [n_words]: positions whose key is not NULL
    uint32_t            elem_size;  // 4 or 8
    const int64_t      *set_keys;   // launch_group_set's outputs
    const uint32_t     *set_slot;
    const uint32_t     *n_found;    // [nq]: the sets' sizes
    uint32_t            k, group_size, km;
    uint64_t           *part_keys;  // [nq][n_part][km], n_part = nprobe * blocks_per_list * 4: the first part_cnt entries of a list are written
    uint32_t           *part_vals;
    uint32_t           *part_slot;
    uint32_t           *part_cnt;   // [nq][n_part]
    const uint32_t     *rank_limit; // as MaskedArgs::rank_limit (pqv_topk_grouped_expand): the lists of a rank at or beyond it go out with part_cnt 0
};
// launch_distinct_stream's walk over the positions whose group value is in the query's set, per-wave lists of at most group_size
// entries per slot (grouped_stream_kernel); StreamArgs::k / part_keys / part_vals are not read
hipError_t launch_grouped_stream(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s);
// the fold of those lists, one wave per query (grouped_merge_kernel)
struct GroupedMergeArgs {
    const uint64_t *part_keys;
    const uint32_t *part_vals;
    const uint32_t *part_slot;
    const uint32_t *part_cnt;
    uint32_t        nq, n_part, k, group_size, km;
    const uint32_t *ids;         // storage row -> reported row (nullptr => identity)
    uint32_t       *row_idx;     // [nq, k, group_size]
    float          *dist;        // [nq, k, group_size]
    uint32_t       *group_rows;  // [nq, k] or nullptr
    int             sqrt_out;    // 0 d2, 1 sqrt(d2), 2 0.5 d2 (PQV_COSINE)
};
hipError_t launch_grouped_merge(const GroupedMergeArgs &a, hipStream_t s);
// group_size == 1 (the distinct call, one row per group): group_rows[q][g] = g < n_found[q] ? 1 : 0
hipError_t launch_group_rows_fill(const uint32_t *n_found, uint32_t nq, uint32_t k, uint32_t *group_rows, hipStream_t s);

// ---- distinct / grouped top-k under a per-query key filter (kernels_distinct_filter.hip; pqv.h: pqv_topk_distinct_filtered) ----
// The filter of such a call: a second key column's position image and the descriptor's device arrays.  kind 0 (PQV_KEY_EQ): a = i64
// [nq] query keys; 1 (PQV_KEY_RANGE): a / b = i64 [nq] inclusive bounds; 2 (PQV_KEY_IN): a = u64 lims [nq + 1], b = i64 values, at
// most KEY_SET_MAX of a query's slice are read.  A position passes iff its filter key is valid and meets the query's test.
struct GroupFilterArgs {
    const void     *key_pos;    // i32 / i64 [n_words * 64]: the filter key of every list position
    const uint64_t *valid_pos;  // optional [n_words]: positions whose filter key is not NULL
    uint32_t        elem_size;  // 4 or 8
    uint32_t        kind;
    const void     *a;
    const void     *b;
};
// launch_distinct_stream / launch_grouped_stream over the positions that also pass fa (distinct_filter_stream_kernel,
// grouped_filter_stream_kernel): the same arguments, outputs and folds
hipError_t launch_distinct_filter_stream(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s);
hipError_t launch_grouped_filter_stream(const StreamArgs &a, const GroupedArgs &ga, const GroupFilterArgs &fa, hipStream_t s);

// ---- predicate masks (kernels_predicate.hip) -----------------------------------------------------------------------------
// A mask's ROW IMAGE is the bitset in row order: bit r of word r / 64 = row r is allowed, ceil(n_rows / 64) words, bits of rows
// >= n_rows zero.  predicate_rows_kernel writes it from resident columns and a postfix program (pqv.h:
// pqv_row_mask_from_predicates; the values below are the header's PQV_COL_* / PQV_OP_* / PQV_PRED_*), mask_pack_kernel from allow
// bytes; mask_gather_kernel turns it into the list-position image and the allowed total, as launch_mask_layout does from bytes.
enum : uint32_t { PRED_COL_I32 = 0, PRED_COL_I64 = 1, PRED_COL_F32 = 2, PRED_COL_F64 = 3 };
enum : uint32_t { PRED_EQ = 0, PRED_NE = 1, PRED_LT = 2, PRED_LE = 3, PRED_GT = 4, PRED_GE = 5, PRED_BETWEEN = 6, PRED_IS_NULL = 7,
                  PRED_MASK = 8, PRED_NOT = 0x100, PRED_PROG_AND = 0x80, PRED_PROG_OR = 0x81 };
struct PredLeaf {
    const void    *values;   // the column's values [n_rows] of dtype; PRED_MASK: the row image of the leaf's mask
    const uint8_t *valid;    // optional validity bytes [n_rows] (0 = NULL)
    uint64_t       a, b;     // operand bits: int64_t (integer columns) / double (float columns)
    uint32_t       op;       // PRED_* | PRED_NOT
    uint32_t       dtype;    // PRED_COL_*
};
struct PredArgs {
    PredLeaf  leaf[32];
    uint32_t  program[16];   // 64 postfix bytes, byte i in bits 8 (i % 4) .. of word i / 4 (a memcpy of the byte program; words, so
                             // that the kernel reads them as scalars): 0..31 push leaf i, PRED_PROG_AND, PRED_PROG_OR (host-checked)
    uint32_t  program_len;
    uint32_t  n_leaves;
    uint64_t  n_rows;
    uint64_t *rowbits;       // [n_words]
    uint64_t  n_words;       // ceil(n_rows / 64)
};
hipError_t launch_predicate_rows(const PredArgs &a, hipStream_t s);
hipError_t launch_mask_gather(const uint64_t *rowbits, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos, uint64_t *bits,
                              uint64_t n_words, unsigned long long *count, hipStream_t s);
hipError_t launch_mask_pack(const uint8_t *allowed, uint64_t n_rows, uint64_t *rowbits, uint64_t n_words, hipStream_t s);

// Batched centroid probe (probe_rows_kernel): every query against every centroid, exact reference order.
struct ProbeRowsArgs {
    const float4   *cent_t;      // [dim/4][kc_pad] float4 transpose of the centroid table (launch_transpose_rows4)
    const float    *queries;     // [nq, dim]
    uint32_t        nq, kc, kc_pad, dim;
    uint64_t       *part_keys;   // [nq][4 * ceil(kc/256)][64], unsorted
    uint32_t       *part_vals;
    uint32_t       *zero_u32;    // optional scratch to zero (as StreamArgs::zero_u32)
    uint32_t        zero_n;
};
hipError_t launch_probe_rows(const ProbeRowsArgs &a, hipStream_t s);
// The same probe, screened (kernels_probe_screen.hip): an f16 contraction of query images against centroid images, bounds of the
// reference distance from every score, exact chains only for the centroids that can be among a query's np nearest.  Writes
// probe_rows_kernel's partial lists, KEY_EMPTY where the bounds exclude a centroid.  The images are launch_center_normalize_f16's
// about ONE vector mu: queries at 2^8 / |q - mu| each, centroids at one table-wide scale cscale.
struct ProbeScreenArgs {
    const uint16_t *q16;         // [nq][dim_p]      f16 images of (q - mu) 2^8 / |q - mu|, dim_p a multiple of 64
    const uint16_t *c16;         // [kc_pad][dim_p]  f16 images of (c - mu) cscale; rows >= kc are zero
    const float    *qn2;         // [nq]  |q - mu|^2 as the image kernel summed it
    const float    *cn2;         // [kc]  |c - mu|^2
    float          *score;       // [nq][kc_pad] scratch
    const float    *queries;     // [nq, dim]
    const float    *centroids;   // [kc, dim] row-major
    uint32_t        nq, kc, kc_pad, dim, dim_p, np;
    // the bound's constants (api.cpp: probe_screen_images)
    float           inv_cs;      // >= 1 / cscale
    float           fn;          // a computed norm times fn is >= the true norm
    float           e1, e2s, kS; // per unit of |a||b|; per unit of |a| (subnormal image components, / cscale); per unit of |a|^2 + |b|^2
    float           lo_f, hi_f;  // 1 -+ the reference chain's margin, rounded outwards
    uint64_t       *part_keys;   // [nq][kc_pad / 64][64], entry c = centroid c
    uint32_t       *part_vals;
    uint32_t       *zero_u32;    // optional scratch to zero (as StreamArgs::zero_u32)
    uint32_t        zero_n;
    unsigned long long *stats;   // diagnostic, optional [3]: += queries, += exact evaluations, += all-exact queries
};
hipError_t launch_probe_screen(const ProbeScreenArgs &a, hipStream_t s);
struct MergeArgs;
// one query: probe + probe merge in one launch (kc_pad <= 4096, nprobe <= 64); the last block to finish merges
// (pr.part_keys: kc_pad keys of scratch; ticket: one zero-initialised u32 that the kernel leaves at zero)
struct PairQuantArgs;
hipError_t launch_probe_single(const ProbeRowsArgs &pr, const MergeArgs &a, uint32_t *ticket, const PairQuantArgs *quant, hipStream_t s);
hipError_t launch_transpose_rows4(const float *rows, uint32_t kc, uint32_t kc_pad, uint32_t dim, void *out, hipStream_t s);

// int8 images of (query, probed list) pairs (kernels_probe.hip: quantize_pair_i8_wave)
struct PairQuantArgs {
    const float    *queries;     // [nq, dim]
    const uint32_t *probe;       // [nq * nprobe] cluster of pair p
    const float    *center;      // [n_clusters, dim]
    const float    *scale;       // [n_clusters]
    const float    *half;        // [n_clusters] largest |x - centre| component of the list
    const float    *radius;      // [n_clusters] upper bound of |x - centre| over the list's rows
    uint32_t        n_pairs, nprobe, dim;
    int8_t         *q_i8;        // [n_pairs, dim]
    int            *q_n2i;       // [n_pairs]
    float          *q_res, *q_resu, *pair_lb;
};

struct MergeArgs {
    const uint64_t *part_keys;   // [nq][n_part][k_part]
    const uint32_t *part_vals;
    uint32_t        nq, n_part, k_part, k;
    // final mode outputs
    const uint32_t *ids;         // storage row -> file row id (nullptr => identity)
    uint32_t       *row_idx;     // [nq, k]
    float          *dist;        // [nq, k]
    uint32_t       *n_found;     // [nq] or nullptr
    int             sqrt_out;    // 0 d2, 1 sqrt(d2), 2 0.5 d2 (PQV_COSINE; tie flags still compare d2)
    uint32_t        k_out;       // results written per query (<= k); 0 => k
    // optional extra source (wide screened path): per-query candidate buffers; with `spilled` the partial
    // lists of a query are read only if spilled[q] != 0
    const uint64_t *cand_keys;   // [nq][cand_cap] or nullptr
    const uint32_t *cand_vals;
    const uint32_t *cand_cnt;    // [nq]
    uint32_t        cand_cap;
    const uint32_t *spilled;     // [nq] or nullptr
    // deferred exact evaluation (TileArgs::cand_lb): the merge first RESOLVES the query's buffer -- T = the k-th smallest upper
    // bound; entries with lower bound <= T are evaluated in the reference's order (index.rs:461-480) against `mat`, the others
    // dropped -- and then merges exact keys as before.  256 threads per query.
    float          *cand_lb;     // [nq][cand_cap] or nullptr
    uint64_t       *cand_keys_rw;
    const float    *mat;         // row-major f32 rows, `dim` values each; cand_vals are row numbers in it
    unsigned long long *resolve_stats;   // optional: the statistics block (slot q % STATS_SLOTS, word 1 += exact evaluations)
    uint32_t       *zero_after;          // final merge: this word is cleared (launch_resolve's work counter, ready for the next call:
                                         // no memset in front of every resolve)
    int             resolve_two_cuts;    // resolve_select_kernel evaluates the entries that define the first cut itself and cuts again (batches:
                                         // the chip is full of such blocks; for a few queries one block per query would be the whole latency)
    uint32_t       *tie_flag;    // [nq] or nullptr: 1 iff two of the first k_out+1 merged entries
                                 // (k_out entries + the runner-up) have equal OUTPUT distance --
                                 // then the reference's order/survivors depend on heap history
    // probe mode outputs (k == nprobe)
    const uint64_t *list_off;
    uint32_t       *probe;       // [nq, k]
    uint64_t       *cand_base;   // [nq, k]
    uint64_t       *n_cand;      // [nq] or nullptr
    uint64_t        max_pos;     // cap applied to n_cand
    // probe mode, optional: the searcher's statistics block -- every query adds its candidate count to the
    // candidate_rows / embeddings_fetched counters (slot q % STATS_SLOTS, words 2 and 3: the plan metrics of
    // src/df_vector/index_exec.rs:289-299 and exec.rs:411-427, kept on the device so that the asynchronous
    // pqv_topk_device path counts too)
    unsigned long long *stats;
    // probe mode extras for the batched path (all optional): cluster histogram of the (query, probe
    // rank) pairs (zeroed beforehand), reset of the per-query admission thresholds, |q|^2
    // one query, nprobe <= 64 (probe mode): the wave also writes the bucketing itself -- every probed cluster is one quad
    // of one pair, in probe-rank order -- and launch_pair_sort is skipped (two launches less per single-query call)
    uint4          *sq_quads;     // nullptr = off
    uint32_t       *sq_pairs, *sq_n_quads;
    uint32_t       *sq_item_quad, *sq_n_items;     // optional work-item table (wide_filter_kernel)
    uint32_t        sq_item_rows, sq_max_items;
    uint32_t       *hist;
    uint32_t        hist_stride;  // > 0: HIST_REPLICAS copies hist[r * hist_stride + c], query q adds to copy q % HIST_REPLICAS
    // probe mode, optional: the query's per-wave partial lists of the re-rank start EMPTY (all-ones keys / values);
    // preset_n entries per query, written by the query's wave (saves a launch per step)
    uint64_t       *preset_keys;
    uint32_t       *preset_vals;
    uint32_t        preset_n;
    // ... or, for the wide screened path (whose waves touch their lists only when a candidate buffer overflows), one
    // "written" byte per list: probe mode clears preset_flag_n bytes per query, wide_filter_kernel sets a list's byte
    // with its first fold (which then writes the whole list), and the final merge reads only flagged lists -- 1 byte per
    // list per step instead of 12 k
    uint8_t        *preset_flags;
    uint32_t        preset_flag_n;
    const uint8_t  *part_flags;  // final mode: [nq][n_part] or nullptr (every list is valid)
    unsigned long long *gthr_init;
    float          *qnorm_out;
    float          *qmax_out;    // max |q_i| per query (f16 screen)
    const float    *queries;
    uint32_t        dim;
    uint32_t       *probe_d2;    // probe mode, optional [nq, k]: the probe distance's bits of every rank, beside `probe` (pqv_topk_depth)
};
hipError_t launch_merge_final(const MergeArgs &a, hipStream_t s);
// deferred evaluations of a BATCH, ahead of launch_merge_final (which then gets cand_lb = nullptr): work = nq * cand_cap uint2 of scratch
hipError_t launch_resolve(const MergeArgs &a, void *work, uint32_t *n_work, bool n_work_is_zero, hipStream_t s);
hipError_t launch_merge_probe(const MergeArgs &a, hipStream_t s);
// table searchers: the probe merge per file segment of the centroid table (kernels_probe.hip: merge_probe_seg_kernel)
struct SegProbeArgs {
    const uint32_t *seg_off;      // [n_files + 1] first global centroid of each file (device)
    uint32_t        n_files, nprobe;
    uint32_t        kmax;         // max over the files of min(nprobe, kc_f) (<= 1024)
    uint32_t        stream_parts; // 0: probe_rows_kernel partials (entry c = centroid c); else stream_kernel partial lists per file
    // round-robin cap (PQV_TABLE_CAP_ROUND_ROBIN, max_cand > 0): file f of query q keeps the first t_f of its c_f candidates, t_f
    // as CandidateCursor::next_batch(max_cand) deals them (access.rs:214-242); pair_end[q * k + j] = the end position of list j's
    // file (its first position + t_f).  file_cnt: [nq * n_files] scratch.  pair_end == nullptr: no cap here.
    uint64_t        max_cand;
    uint32_t       *file_cnt;
    uint64_t       *pair_end;
};
hipError_t launch_merge_probe_seg(const MergeArgs &a, const SegProbeArgs &g, hipStream_t s);
// stream_kernel arguments of the per-file centroid pass: probe[q * n_files + f] = f, cand_base[...] = seg_off[f]
hipError_t launch_seg_probe_fill(const uint32_t *seg_off, uint32_t n_files, uint32_t nq, uint32_t *probe, uint64_t *cand_base, hipStream_t s);

// ---- batched re-rank: cluster-major tiles ------------------------------------------------
// The (query, probe-rank) pairs of a batch are bucketed by cluster; a "group" is up to
// TILE_QB pairs of one cluster.  tile_rerank streams each row tile of that cluster ONCE for
// the whole group (queries as wave-uniform scalar operands), instead of once per query.
constexpr int TILE_QB = 16;

constexpr uint32_t HIST_REPLICAS = 16;
// statistics counters live in STATS_SLOTS copies one cache line apart: stats[8 + 16 i + {0, 1}] screened pairs /
// survivors (wide_filter_kernel), + {2, 3} candidate rows / embeddings fetched (probe merge)
constexpr uint32_t STATS_SLOTS = 64;

constexpr uint32_t ITEM_LEVELS = 64;
struct PairSortArgs {
    const uint32_t *probe;     // [nq * nprobe] cluster of pair p = q*nprobe + j
    uint32_t        n_pairs, n_clusters;
    int             hist_done; // 1: hist was already filled (launch_merge_probe with MergeArgs::hist)
    uint32_t       *hist;      // [n_clusters]      (zeroed by the caller)
    uint32_t        hist_stride; // > 0: the histogram arrives as HIST_REPLICAS partial copies, stride apart; the scan sums
                                 //      them into copy 0 (8 k atomics on the four lines of one copy serialise: 20 -> 9 us on C2)
    uint32_t       *cursor;    // [n_clusters] zeroed by the caller; with hist_stride > 0: [HIST_REPLICAS][hist_stride], set by the
                               // scan to each copy's first index in its cluster's bucket (the scatter's atomics spread likewise)
    uint32_t        nprobe;    // pairs per query (pair p belongs to query p / nprobe: selects the copy)
    uint32_t       *pair_off;  // [n_clusters + 1]
    uint32_t       *group_off; // [n_clusters + 1]
    uint32_t       *pairs;     // [n_pairs] pair ids bucketed by cluster
    uint4          *groups;    // [max_groups] {cluster, first slot, count, 0}
    uint32_t       *n_groups;  // [1]
    // quads: up to quad_width (32 or 64) pairs of one cluster (the unit of wide_filter_kernel)
    uint32_t        quad_width;
    uint32_t       *quad_off;  // [n_clusters + 1]
    uint4          *quads;     // [max_quads] {cluster, first slot, count, 0}
    uint32_t       *n_quads;   // [1]
    // optional work-item table of the wide filter kernel: one item per (quad, row chunk that exists in the quad's
    // list), quads in order, so that the kernel's 1-D grid holds no empty workgroups between real ones
    const uint64_t *list_off;  // [n_clusters + 1]
    uint32_t        item_rows; // rows per chunk (the kernel's rows_per_block); 0 = no table
    uint32_t       *item_off;  // [n_clusters + 1] first item of each cluster's first quad
    uint32_t       *n_items;   // [1]
    uint32_t       *item_quad; // [max_items] quad of each item; quads[q].w = the quad's first item
    uint32_t        max_items;
    // chunk-major item order (item_chunk != nullptr): items are numbered level by level -- row chunk 0 of every quad, then
    // chunk 1, ... (levels >= ITEM_LEVELS - 1 share the last one) -- so a query's thresholds have seen the first chunk of
    // all its lists before any later chunk is screened.  pair_scan_kernel writes the tables (order inside a level: by cluster).
    uint32_t       *item_chunk;      // [max_items] row chunk of each item
    uint32_t       *wide_item_chunk; // [wide_max_items]
    uint32_t       *wide_stats;      // optional [2]: items of the wide table, and how many of them belong to lists with no other quad
    uint32_t       *shape_stats;     // optional [2] (pinned host memory): rows of the lists that more than shape_wide pairs of the batch
    uint32_t        shape_wide;      // probe, and of those that more than shape_narrow do -- how the next batch cuts its quads
    uint32_t        shape_narrow;    // (its own width: quad_width is the 160-wide cut while the wide-quad instance is active)
    uint32_t        wide_list_major; // the WIDE table keeps list-major order (a list's chunks are consecutive items: pair_scatter_kernel writes
                                     // them, wide_item_chunk stays unused) while the regular one is chunk-major -- list_filter_kernel maps
                                     // consecutive items to ONE XCD, whose L2 then holds the list's pair images for all of its chunks
    uint32_t        xcd_items;       // bit 0: the regular table, bit 1: the wide table -- a level's slots filled column by column of an
                                     // 8-column layout (the quads of one list -> the same XCD, back to back)
    // optional second class of quads (the wide-quad instance of the filter kernel): with wide_min > 0 the quads are cut
    // quad_width (160) pairs wide, and a quad of >= wide_min (97) pairs is WIDE -- its items (chunks of wide_item_rows rows)
    // go to a table of their own, quads[q].w = its first item THERE; the others (<= 96 pairs: one per list at most, the
    // last) stay in item_quad
    uint32_t        wide_min;
    uint32_t        wide_item_rows;
    uint32_t       *wide_item_off;  // [n_clusters + 1]
    uint32_t       *wide_n_items;   // [1]
    uint32_t       *wide_item_quad; // [wide_max_items]
    uint32_t        wide_max_items;
    // optional [n_pairs / nprobe] (pqv_topk_depth): pair (q, j) with j >= rank_limit[q] is left out of the scatter, as
    // probe_depth_kernel left it out of the histogram -- no group, quad or work item exists for a rank nobody walks
    const uint32_t *rank_limit;
};
// hist -> scan -> scatter; three tiny launches
hipError_t launch_pair_sort(const PairSortArgs &a, hipStream_t s);

// Optional refinement of the seed threshold (k <= 16, dim % 32 == 0): the k sampled bounds a query selects belong to 4 k
// rows (a bound is a lane's minimum over the 4 sub-tile rows it saw); their EXACT reference distances are evaluated
// and the k-th smallest of those -- still k distinct candidates, so still an upper bound of the final k-th distance --
// replaces the k-th bound: the threshold loses the slack of the operand form (int8: ~1 % of d2) before the screen starts.
struct SeedRefine {
    const float    *mat;        // f32 rows [*, dim] (nullptr = no refinement): list position p is storage row row_of ? row_of[p] : p
    const uint32_t *row_of;
    const float    *queries;    // [nq, dim]
    const uint64_t *list_off;
    const uint32_t *probe;      // [nq, nprobe]
    const uint64_t *cand_base;  // [nq, nprobe]
    uint32_t        dim, nprobe, seed_sw, seed_rows;
    uint64_t        max_pos;
    const uint64_t *pair_end;   // [nq, nprobe] or nullptr (StreamArgs::pair_end)
};
// One-query calls: wide_seed_kernel's LAST block to finish (a ticket counter) runs seed_select_kernel's body itself.
struct SeedTail {
    int                 enable;
    uint32_t            n_vals, k;
    unsigned long long *gthr;
    uint32_t           *cand_cnt, *spilled, *thr_hist;
    float4             *thr_bins;
    uint32_t           *ticket;      // zero-initialised, left at zero
    uint32_t            lds_floats;  // dynamic LDS of the launch, in floats (set by launch_wide_seed): the refinement's term table
    SeedRefine          rf;
};
struct TileArgs {
    const float    *mat;
    const uint32_t *row_of;
    const uint64_t *list_off;
    const float    *queries;
    const uint64_t *cand_base;   // [nq * nprobe]
    const uint32_t *pairs;
    const uint4    *groups;
    const uint32_t *n_groups;
    uint32_t        max_groups;  // gridDim.y
    const uint4    *quads;       // wide_filter_kernel: gridDim.y = max_quads
    const uint32_t *n_quads;
    uint32_t        max_quads, quad_width;
    uint32_t        block_waves; // wide_filter_kernel: waves per block, 4 (default when 0) or 8 (one block per CU sharing a staged quad of up to 128 queries)
    uint32_t        nq, nprobe, dim, k;
    uint32_t        rows_per_block, blocks_per_list;
    uint64_t        max_pos;
    const uint64_t *pair_end;    // [nq * nprobe] or nullptr: the pair's candidates end there instead (StreamArgs::pair_end)
    unsigned long long *gthr;    // [nq] per-query global admission threshold, preset to KEY_EMPTY
    // row window of this launch inside every list: rows [row_offset, row_offset + gridDim.x *
    // rows_per_block).  Partial-list slots: a (query, probe rank j) pair owns slots_per_pair
    // lists; block bx of this launch writes slots slot_base + bx * 4 + wave (one list per wave)
    uint64_t        row_offset;
    uint64_t        row_end;     // 0 = none: rows at list offsets >= row_end belong to a later launch
    uint32_t        slots_per_pair, slot_base;
    uint32_t        n_part;      // partial lists per query in part_keys (>= nprobe * slots_per_pair)
    uint32_t        grid_x;      // gridDim.x of this launch
    int             filter_variant;   // launch_tile_filter: 0 = wide_filter_kernel (2 or 4 query groups per block,
                                      // queries staged in LDS), 1 = tile_filter_kernel (one group per block)
    // MFMA filter only: squared norms of the storage rows / of the queries
    const float4   *mat_blk;     // wide_filter_kernel: blocked copy of the IVF-ordered lists (launch_block_rows)
    const uint64_t *blk_off;     // [n_clusters + 1] first 16-row tile of every list in mat_blk
    // f16 operands (wide kernels, dim % 128 == 0): mat_blk is the launch_block_rows_f16 copy, the queries are
    // converted while staged; scale is a power of two, scale2 = scale^2
    int             f16;
    int             q32_lds;      // set by the launcher: the f16 kernel also stages the exact f32 queries in LDS
    float           scale, scale2;
    const float    *query_maxabs;   // [nq] max |q_i| (merge probe)
    // int8 operands (wide kernels, dim % 256 == 0): mat_blk is the launch_block_rows_i8 copy -- per list the residual
    // against the list's centre at the list's scale; the query side is one image per (query, probed list) PAIR
    // (launch_quantize_pairs_i8), indexed by pair = query * nprobe + probe rank
    int             i8;
    const int8_t   *q_i8;        // [nq * nprobe][dim]
    const int      *q_n2i;       // [nq * nprobe] |vi|^2
    const float    *q_res;       // [nq * nprobe] rounding residual of the clamped query residual (lower bounds; +inf: never skip)
    int             i8_pair_images;   // 1: images per pair (the residual form); 0: ONE image per query, indexed by query (every
                                      // list shares centre and scale: the tables hold the same values for all lists)
    const float    *q_resu;      // [nq * nprobe] ... plus what the clamp cut off (upper bounds: wide_seed_kernel)
    const float    *pair_lb;     // [nq * nprobe] or nullptr: lower bound of d2(query, any row of the pair's list)
    const float    *list_scale;  // [n_clusters] S_c
    const int      *row_n2i;     // per storage row: |xi|^2
    const float    *row_res;     // per storage row: upper bound of |x - c - xi / S|
    const float4   *q_blk;       // wide kernels without LDS staging (long rows): blocked queries per quad
                                 // (launch_pack_queries), [max_quads][quad_width / 16][dim / 4][16] float4
    const float    *row_norm2;   // indexed like mat rows (norm_by_pos: by LIST POSITION -- images in list order over row-order f32 rows)
    int             norm_by_pos;
    const float    *query_norm2; // [nq]
    int             xcd_swizzle; // 1: XCD-aware workgroup remap (speed only)
    const uint32_t *item_quad;   // wide_filter_kernel: work-item table (PairSortArgs::item_quad); nullptr = 2-D grid
    const uint32_t *n_items;
    uint32_t        max_items;
    // second launch for the WIDE quads (PairSortArgs::wide_*): 8-wave blocks, quads of wide_width queries on 32-row tiles
    uint32_t        wide_width;  // 0 = none
    const uint32_t *wide_item_quad;
    const uint32_t *item_chunk, *wide_item_chunk;   // chunk-major tables (PairSortArgs::item_chunk); nullptr = chunk = item - quads[q].w
    uint32_t        wide_nt;         // the wide-quad instance streams its rows with the nt policy (most of its lists have one quad)
    uint32_t        list_once;       // the wide table's quads (up to wide_width <= 1024 pairs of one list) run in list_filter_kernel (kernels_list.hip)
    // host side only (launch_tile_filter): run the wide-quad instance on `side_stream`, forked from and joined to the call's stream
    // by the two events, so that the two instances' tails fill each other (they cannot share a CU -- 2 x 81 KB against 142 KB
    // of LDS -- but they can share the chip); NULL: one after the other on the call's stream
    uint32_t        opt_pf96;        // f16 96-query form on rows of <= 128 dims: whole-tile operand prefetch (PQV_PF96)
    uint32_t        static_dim;      // int8 instances of the batched dispatch: the row length compiled in where it was instantiated (768)
    uint32_t        drain_min;       // wide_filter_kernel: queue entries that start a batch of exact evaluations before the wave's last tile (0 = 64)
    hipStream_t     side_stream;
    hipEvent_t      ev_fork, ev_join;
    uint32_t        fork_wide_first; // the wide-quad launch is enqueued first, on the call's stream; the regular one on the side stream
    const uint32_t *wide_n_items;
    uint32_t        wide_max_items, wide_rows_per_block;
    // wide_filter_kernel: per-query append buffers of exact-verified candidates
    uint64_t       *cand_keys;   // [nq][cand_cap]
    uint32_t       *cand_vals;
    uint32_t       *cand_cnt;    // [nq] appended so far (may exceed cand_cap: the excess went to the wave lists)
    uint32_t        cand_cap;
    uint32_t       *spilled;     // [nq] set to 1 when a query overflowed its buffer
    // DEFERRED exact evaluation (optional): a survivor of the screen is appended with the BOUNDS its screen score gives --
    // key = (upper bound of the reference distance << 32 | position), cand_lb = lower bound -- instead of being evaluated by
    // the streaming wave; the final merge evaluates only the entries whose lower bound does not exceed the k-th smallest upper
    // bound of the query (MergeArgs::cand_lb).  cand_lb < 0 marks an entry whose key already holds the exact distance (pairs
    // without usable bounds: non-finite data, f16 range overflow, a tile with too many survivors for one expansion pass).
    float          *cand_lb;     // [nq][cand_cap] or nullptr (evaluate in the filter)
    uint32_t       *pendv;       // scratch [blocks][waves][wide_filter_pend()]: raw screen scores of the queued survivors
    uint32_t       *pendv_wide;  // ... of the wide-quad instance's launch
    // wide_seed_kernel: upper bounds [nq][nprobe][seed_sw][16], seed_sw = 4 * gridDim.x of the seed launch
    float          *seed_ub;
    SeedTail        seed_tail;   // wide_seed_kernel, one query: select + refine in the same launch
    uint32_t        seed_sw;
    // running thresholds (wide_filter_kernel, optional): per query two 64-bit words of 8-bit counters --
    // counter b = appended pairs at distance < thr0 - b w -- and the bin parameters {thr0, w, 1 / w, pad}
    // (seed_select_kernel); an appending lane tightens gthr[q] to the upper edge of the nearest bin whose
    // counter reached k
    uint32_t       *thr_hist;
    const float4   *thr_bins;
    unsigned long long *stats;   // [2] optional: += (row, query) pairs screened, += pairs evaluated exactly
    uint64_t       *part_keys;   // [nq][nprobe * slots_per_pair][k]
    uint32_t       *part_vals;
    uint8_t        *part_flags;  // wide_filter_kernel, optional: [nq][n_part] "this list has been written" (see MergeArgs)
};
// PQV_L2SQ_REF4 only, k <= 256.  The caller presets the whole partial-list buffer to EMPTY (0xFF bytes:
// KEY_EMPTY keys, 0xFFFFFFFF values); a wave touches its slots only when a candidate is admitted.
hipError_t launch_tile_rerank(const TileArgs &a, hipStream_t s);
// entries of a wave's survivor queue in wide_filter_kernel<NG = quad_width / 16, NW = waves> (TileArgs::pendv is sized with it)
constexpr uint32_t wide_filter_pend(uint32_t quad_width, uint32_t waves, bool f16) {
    return (waves == 8 ? (quad_width == 64 && f16 ? 512u : 256u) : quad_width == 96 ? 128u : 512u) + 64u;
}
// Same contract, but every (row, query) pair is first screened with an MFMA lower bound of its
// distance; only pairs that could still beat the query's admission threshold are evaluated in
// the reference's exact order.  Needs thresholds seeded by a prior launch_tile_rerank window.
hipError_t launch_tile_filter(const TileArgs &a, hipStream_t s);
// The row-stationary int8 screen for the lists that many queries of the batch probe (kernels_list.hip): `a` is the wide table's
// view of the step -- item_quad / item_chunk / n_items / max_items / rows_per_block of THAT table, quads of up to 1024 pairs.
hipError_t launch_list_filter(const TileArgs &a, hipStream_t s);
// After the exact seed window: gthr[q] = min(gthr[q], k-th smallest key over ALL of q's seed lists)
// (slots 0..3 of every (query, probe rank) pair) -- the k-th of the union, far tighter than the min
// of the per-wave k-th keys the fold publishes.
hipError_t launch_seed_threshold(const uint64_t *part_keys, uint32_t nq, uint32_t nprobe, uint32_t slots_per_pair,
                                 uint32_t k, unsigned long long *gthr, hipStream_t s);

// Thresholds of the wide screened pass from MFMA upper bounds (no exact seed pass): launch_wide_seed over
// the first rows of every list fills TileArgs::seed_ub, launch_seed_select turns a query's n_vals =
// nprobe * seed_sw * 16 minima into gthr[q] and resets its candidate buffer / overflow flag.
hipError_t launch_wide_seed(const TileArgs &a, hipStream_t s);
hipError_t launch_seed_select(const float *seed_ub, uint32_t nq, uint32_t n_vals, uint32_t k, unsigned long long *gthr,
                              uint32_t *cand_cnt, uint32_t *spilled, hipStream_t s,
                              uint32_t *thr_hist = nullptr, float4 *thr_bins = nullptr, const SeedRefine *refine = nullptr,
                              const uint32_t *rank_limit = nullptr, uint32_t per_rank = 0);
// (rank_limit, optional [nq] with per_rank = the bounds per probe rank, pqv_topk_depth: query q selects among the bounds of its
//  ranks below rank_limit[q] only -- the first rank_limit[q] * per_rank of its n_vals)

// ---- batched brute force as a dense Q.V^T contraction on f32 MFMA (BASELINE config 5) -------
// score s[i][j] = q_i . v_j over ALL rows j of a row range; distance by `metric`:
//   BRUTE_COSINE : d = 1 - s * rq[i] * rv[j]     (rq, rv = reciprocal L2 norms)
//   BRUTE_L2SQ   : d = max(0, qn[i] + vn[j] - 2 s)   (norm-expansion form: NOT the reference's
//                  summation order -- tolerance-level agreement only)
// Candidates whose key beats the query's current threshold are appended to a per-query buffer.
enum BruteMetric : int { BRUTE_COSINE = 0, BRUTE_L2SQ = 1 };

struct BruteArgs {
    const float *rows;        // [n, dim]
    const float *queries;     // [nq, dim]
    const float *row_aux;     // [n]  rv (cosine) or vn (l2)
    const float *query_aux;   // [nq] rq or qn
    uint64_t     row_begin, row_end;   // row range of this launch
    uint32_t     nq, dim;
    int          metric;
    const unsigned long long *thr;     // [nq] admission threshold (sortable key), KEY_EMPTY = none
    unsigned long long *cand;          // [nq][cap] appended keys
    uint32_t    *cand_cnt;             // [nq]
    uint32_t     cap;
    // dense != 0: no thresholds yet and empty buffers (the first row range): EVERY pair is kept, in slot row - row_begin of
    // its query -- no atomic per pair; the caller sets cand_cnt to the range's length (<= cap) afterwards
    uint32_t     dense;
};
hipError_t launch_brute_mfma(const BruteArgs &a, hipStream_t s);
// The f16 screen of the same search (kernels_brute.hip: brute_f16_kernel): L2-normalised f16 images x 2^8 of rows / queries
// ([*, dim_p], dim_p a multiple of 32, launch_normalize_f16), lower-bound keys against the exact thresholds; appended
// entries are then rewritten with their exact f32 keys by launch_brute_rescore (entries [first[q], cand_cnt[q]) of query q).
struct BruteF16Args {
    const uint16_t *v16;       // [n, dim_p]
    const uint16_t *q16;       // [nq, dim_p]
    // int8 form (v8 != nullptr; dim_p a multiple of 64): images of (unit vector - its mid-range) and per vector
    // {1 / S, residual norm, mid-range, component sum} + |unit vector - mid-range| (launch_normalize_i8); eps then carries only
    // the f32 roundings (eps_sum: of the component sums, per unit of |mid-range|) -- the image bound is per pair
    const int8_t   *v8, *q8;
    const float4   *row_sr, *query_sr;
    const float    *row_n, *query_n;
    const float    *row_max;  // [9] corpus-wide maxima of |sum - mid-range dim|, norm + 3 residual, |mid-range|, residual, 1 / S, and -- as
                              // sortable_bits keys -- of C, -C, A, -A (C = mid-range, A = sum - mid-range dim): the epilogue's screens
    float           dim_f, eps_sum;
    const float *row_aux;      // [n]  |v|^2 (l2 only)
    const float *query_aux;    // [nq] |q|^2 (l2 only)
    uint64_t     row_begin, row_end;
    uint32_t     nq, dim_p;
    int          metric;
    float        eps;          // bound of |s~ - s^| on the cosine scale
    const unsigned long long *thr;
    unsigned long long *cand;
    uint32_t    *cand_cnt;
    uint32_t     cap;
};
hipError_t launch_brute_f16(const BruteF16Args &a, hipStream_t s);
// The k-means assignment on the f16 matrix pipe (kernels_build.hip: assign_f16_kernel): images of (row - mu) / |row - mu| * 2^8
// for rows and centroids (launch_center_normalize_f16; the centroid table padded to kc_pad rows, a multiple of 256),
// candidate lists per row, then launch_assign_rescore picks the exact argmin among them.
struct AssignF16Args {
    const uint16_t *x16;     // [m, dim_p]
    const uint16_t *c16;     // [kc_pad, dim_p]
    const float    *xn2;     // [m]  |row - mu|^2
    const float    *cn2;     // [kc] |centroid - mu|^2
    uint64_t        m;
    uint32_t        kc, kc_pad, dim_p;
    float           eps, cm;  // image dot-product bound (cosine scale); the reference summation margin
    uint32_t       *cand;     // [m][cap] candidate centroid ids
    uint32_t       *cand_cnt; // [m] (zeroed by the caller; may exceed cap: the row is then compared with every centroid)
    uint32_t        cap;
};
hipError_t launch_assign_f16(const AssignF16Args &a, hipStream_t s);
// Round 4 form of the same screen (kernels_build.hip: assign_wide_kernel): block tile 256 rows x 256 centroids (8 waves, 128-byte K
// stages), the data rows on the LANE-owned side of the MFMA so that a row's running best needs no cross-lane reduction, centroid
// images at ONE global scale (cscale = 2^8 / max |c - mu|) so that the whole epilogue of a pair is  t = cn2[c] - kA xs acc  (one
// FMA + one min; d~ = |x - mu|^2 + t).  Candidates carry their t; launch_assign_resolve filters them against the row's FINAL
// best (the kernel's own test only sees the best so far), returns the survivor where one is left and evaluates exactly --
// reference order, argmin by (distance bits, index) -- only the rows that keep two or more.
struct AssignWideArgs {
    const uint16_t *x16;     // [m, dim_p] images of (row - mu) / |row - mu| * 2^8, dim_p a multiple of 64
    const uint16_t *c16;     // [kc_pad, dim_p] images of (centroid - mu) * cscale; rows >= kc are zero
    const float    *xn2;     // [m]  |row - mu|^2
    const float    *cn2;     // [kc] |centroid - mu|^2   (c16 / cn2 in SORTED order: ascending norm; perm[s] = the centroid in slot s)
    const uint32_t *perm;    // [kc]
    const float    *grp_cs;  // [kc_pad / 32] per group of 32 sorted centroids: >= max |c - mu| ...
    const float    *grp_cn;  // [kc_pad / 32] ... and >= max cn2 (a group's own maxima scale its error bound, not the table's: the
                             // few far-out centroids -- clusters of one or two sample points -- loosen only their own group)
    uint64_t        m;
    uint32_t        kc, kc_pad, dim_p;
    float           kA;      // 2 / (2^8 cscale): (row - mu).(centroid - mu) = acc |row - mu| kA / 2
    float           eps, cm;
    uint32_t       *cand;     // [m][cap] candidate centroid ids
    float          *cand_t;   // [m][cap] their lower-bound scores t - E
    uint32_t       *cand_cnt; // [m] zeroed by the caller; may exceed cap (the row is then compared with every centroid)
    float          *best_t;   // [m] smallest upper-bound score t + E of the row over all centroids
    uint32_t        cap;
};
hipError_t launch_assign_wide(const AssignWideArgs &a, hipStream_t s);
hipError_t launch_assign_resolve(const AssignWideArgs &a, const float *rows, const float *centroids, uint32_t dim, uint32_t *cluster,
                                 unsigned long long *stats /* optional [2]: += rows evaluated exactly, += exact evaluations */, hipStream_t s);
hipError_t launch_assign_rescore(const float *rows, const float *centroids, uint64_t m, uint32_t dim, uint32_t kc, const uint32_t *cand,
                                 const uint32_t *cand_cnt, uint32_t cap, uint32_t *cluster, hipStream_t s);
// fixed_scale > 0: every row is multiplied by that one scale instead of 2^8 / its own norm (the centroid images of the round-4 form)
// idx != nullptr: output row r is made from rows[idx[r]]
hipError_t launch_center_normalize_f16(const float *rows, const float *mu, uint64_t n, uint64_t n_pad, uint32_t dim, uint32_t dim_p,
                                       float *out_n2, void *out, hipStream_t s, float fixed_scale = 0.0f, const uint32_t *idx = nullptr);
// the longest chain of f32 roundings behind an out_n2 value of that kernel (fused multiply-adds of a lane, then the wave's tree):
// a sum of non-negative terms is within that many units of 2^-24, relatively, of the exact one
uint32_t center_normalize_f16_sum_depth(uint32_t dim);
hipError_t launch_col_mean(const float *m, uint32_t k, uint32_t dim, float *mu, hipStream_t s);
hipError_t launch_normalize_f16(const float *rows, const float *rnorm, uint64_t n, uint32_t dim, uint32_t dim_p, void *out, hipStream_t s);
hipError_t launch_normalize_i8(const float *rows, const float *rnorm, uint64_t n, uint32_t dim, uint32_t dim_p, void *out, void *sr, float *nrm,
                               float *maxima /* [9], zeroed by the caller; nullptr: not wanted */, hipStream_t s);
hipError_t launch_brute_rescore(const BruteArgs &a, const uint32_t *first, hipStream_t s);
// per-row auxiliary values: mode 0 = 1/sqrt(sum x^2) (0 for a zero row), mode 1 = sum x^2, mode 2 = max |x_i|
hipError_t launch_row_norms(const float *rows, uint64_t n, uint32_t dim, int mode, float *out, hipStream_t s);
// fold a query's appended candidates to its k best (kept at the front of the buffer), set
// thr[q] to its k-th key once k candidates exist, report overflow (count > cap) in *overflow
hipError_t launch_brute_select(unsigned long long *cand, uint32_t *cand_cnt, uint32_t cap, uint32_t nq,
                               uint32_t k, unsigned long long *thr, uint32_t *overflow, hipStream_t s);
// *overflow |= 1 if any query's appended count exceeds cap (run BEFORE the select pass, which
// rewrites the buffer fronts)
hipError_t launch_brute_overflow_check(const uint32_t *cand_cnt, uint32_t nq, uint32_t cap, uint32_t *overflow,
                                       hipStream_t s);
// decode the k best keys of every query: row ids + distances
hipError_t launch_brute_finish(const unsigned long long *cand, const uint32_t *cand_cnt, uint32_t cap,
                               uint32_t nq, uint32_t k, uint32_t *row_idx, float *dist, uint32_t *n_found,
                               hipStream_t s);

// Merge of per-shard top-k lists gathered from all ranks: dist/rows [n_shards, nq, k] (unused
// slots: +inf / 0xFFFFFFFF), row_base[n_shards] the shards' first global row.  One wave per
// query; order = ascending (distance, shard, position in the shard's list).
// `stride` = elements between consecutive results in dist / rows (1: two dense arrays; 2: one packed array of
// {f32 distance, u32 row} pairs, dist = base, rows = base + 1)
hipError_t launch_shard_merge(const float *dist, const uint32_t *rows, const long long *row_base,
                              uint32_t n_shards, uint32_t nq, uint32_t k, float *out_dist,
                              long long *out_rows, hipStream_t s, uint32_t stride = 1);

// out[i] = {bits of dist[i], rows[i]} (8 bytes per result): the packed form pqv_merge_topk_packed_device reads
hipError_t launch_pack_pairs(const float *dist, const uint32_t *rows, uint64_t n, void *out, hipStream_t s);

// MFMA-operand copy of the IVF-ordered lists: 16-row tiles, tile T column ch row j at float4 index
// (T * dim/4 + ch) * 16 + j; blk_off[c] = first tile of list c (lists are padded to 16 rows with zeros)
// (row_of, here and below: list position p reads source row row_of[p]; nullptr = the source is already in list order)
hipError_t launch_block_rows(const float *src, const uint64_t *list_off, const uint64_t *blk_off, uint32_t n_clusters,
                             uint64_t max_tiles, uint32_t dim, void *out, hipStream_t s, const uint32_t *row_of = nullptr);

// blocked copy of every quad's queries (see TileArgs::q_blk); ngrp = quad_width / 16
hipError_t launch_pack_queries(const float *queries, const uint32_t *pairs, const uint4 *quads, const uint32_t *n_quads,
                               uint32_t max_quads, uint32_t nprobe, uint32_t dim, uint32_t ngrp, void *q_blk, hipStream_t s);

// MFMA-screened assignment helpers (api.cpp: assign_screened).  assign_setup: pairs[i] = i, quads of `width`
// consecutive queries of cluster 0, cand_base = 0, gthr = EMPTY, *n_quads.  nonfinite_flag: *flag |= 1 if any
// v[i] is inf / NaN.  count_changed: *changed += #{i : cur[i] != prev[i]}.
hipError_t launch_assign_setup(uint32_t *pairs, uint4 *quads, uint32_t *n_quads, uint64_t *cand_base, unsigned long long *gthr,
                               uint32_t nq, uint32_t width, hipStream_t s);
hipError_t launch_nonfinite_flag(const float *v, uint64_t n, uint32_t *flag, hipStream_t s);
// The inverted lists on the device (kernels_build.hip: list_*_kernel): a stable counting sort of the rows by cluster -- list c holds
// the row ids assigned to c in ascending order (index.rs:193-206).  cnt: scratch [k][ceil(n / rows_per_block)] u32, tot: scratch [k] u64,
// list_off: [k + 1] u64, list_rows: [n] u32, *bad: set to 1 if an assignment is >= k (preset 0).  k <= 4096, n < 2^32,
// rows_per_block a multiple of 256.
hipError_t launch_list_sort(const uint32_t *assign, uint64_t n, uint32_t k, uint32_t *cnt, uint32_t rows_per_block,
                            unsigned long long *tot, uint64_t *list_off, uint32_t *list_rows, uint32_t *bad, hipStream_t s);
// The lists of an index extended by a sorted range of new rows (kernels_append.hip: list_splice_kernel; pqv_index_append):
// out_off[c] = old_off[c] + add_off[c] for c in [0, k], out_rows[out_off[c] ..) = old list c verbatim, then first_row + add_rows[add_off[c] ..)
// (add_off / add_rows: launch_list_sort over the range, ids local to it).  total = old_off[k] + add_off[k] entries of out_rows (16-byte
// aligned); old_rows may be NULL where the old lists are empty.  k <= 4096.
hipError_t launch_list_splice(const uint64_t *old_off, const uint32_t *old_rows, const uint64_t *add_off, const uint32_t *add_rows,
                              uint32_t k, uint32_t first_row, uint64_t total, uint64_t *out_off, uint32_t *out_rows, hipStream_t s);
// Ranking over a bitset (kernels_remove.hip; pqv_index_remove / pqv_index_compact).  A bitset of n_bits bits is ceil(n_bits / 64)
// words; `invert` reads the stored bits as "leaves" (launch_mask_layout's image of the remove flags), bits at or beyond n_bits never
// count.  launch_bit_rank: rank[w] = set bits of the words before w, rank[ceil(n_bits / 64)] = the total (rank holds one entry more
// than the words); block_tmp holds bit_rank_blocks(n_bits) + 1 u64.
uint64_t bit_rank_blocks(uint64_t n_bits);
hipError_t launch_bit_rank(const uint64_t *bits, uint64_t n_bits, bool invert, uint64_t *rank, uint64_t *block_tmp, hipStream_t s);
// out[set bits below p] = ids ? ids[p] : p for every set position p < n_pos (<= 2^32), order kept; out holds the total
hipError_t launch_list_compact(const uint32_t *ids, uint64_t n_pos, const uint64_t *bits, bool invert, const uint64_t *rank, uint32_t *out,
                               hipStream_t s);
// new_off[c] = set bits below position old_off[c] (old_off[c] <= n_pos), c in [0, n_entries)
hipError_t launch_offsets_rank(const uint64_t *old_off, uint32_t n_entries, const uint64_t *bits, uint64_t n_pos, bool invert,
                               const uint64_t *rank, uint64_t *new_off, hipStream_t s);
// member[ids[p]] = 1 (member: n_rows zeroed bytes); *bad |= 1 where an id is >= n_rows (nothing is written for it)
hipError_t launch_member_bytes(const uint32_t *ids, uint64_t n_pos, uint64_t n_rows, uint8_t *member, uint32_t *bad, hipStream_t s);
// out[p] = set bits of rowbits below ids[p] (rowbits / rank over n_rows row ids; out 16-byte aligned)
hipError_t launch_lists_remap(const uint32_t *ids, uint64_t n_pos, const uint64_t *rowbits, uint64_t n_rows, const uint64_t *rank,
                              uint32_t *out, hipStream_t s);
// dst[j, :] = src[old_row[j], :] for j < m, bit for bit (every old_row[j] is a row of src)
hipError_t launch_rows_gather(const float *src, const uint32_t *old_row, uint64_t m, uint32_t dim, float *dst, hipStream_t s);
hipError_t launch_count_changed(const uint32_t *cur, const uint32_t *prev, uint64_t n, unsigned long long *changed, hipStream_t s);

// pqv_rerank's running state <-> merge lists (see kernels_layout.hip)
hipError_t launch_rerank_state_in(const uint32_t *io_rows, const float *io_d2, const uint32_t *io_count, uint32_t k, uint32_t k_list,
                                  uint64_t *keys, uint32_t *vals, uint32_t *rows_saved, hipStream_t s);
hipError_t launch_rerank_state_out(const uint32_t *m_vals, const float *m_d2, const uint32_t *m_found, const uint32_t *rows_saved,
                                   const uint32_t *ids, uint32_t k, uint32_t *io_rows, float *io_d2, uint32_t *io_count,
                                   const uint32_t *m_tie, uint32_t *io_tie, hipStream_t s);

// a[0 .. a_bytes) and b[0 .. b_bytes) = 0xFF bytes in one launch (byte counts: multiples of 16)
hipError_t launch_fill_ones2(void *a, uint64_t a_bytes, void *b, uint64_t b_bytes, hipStream_t s);

// f16 form of the blocked copy (values * scale rounded to nearest f16, 8 dims per 16-byte column, tile T column
// cc row j at 16-byte index (T * dim/8 + cc) * 16 + j) and the corpus maximum it is scaled by
hipError_t launch_block_rows_f16(const float *src, const uint64_t *list_off, const uint64_t *blk_off, uint32_t n_clusters,
                                 uint64_t max_tiles, uint32_t dim, float scale, void *out, hipStream_t s, const uint32_t *row_of = nullptr);
hipError_t launch_maxabs(const float *v, uint64_t n, uint32_t *out_bits, hipStream_t s);
// one pass over n rows (row r = source row row_of ? row_of[r] : r): out_norm2[r] = sum x^2 and *max_bits = max(*max_bits, bits(max |x|))
hipError_t launch_row_norms_max(const float *rows, const uint32_t *row_of, uint64_t n, uint32_t dim, float *out_norm2, uint32_t *max_bits,
                                hipStream_t s);
// int8 form (see kernels_layout.hip): per-list, per-dimension min / max keys (kmin preset to 0xFF bytes, kmax to 0; [n_clusters, dim]),
// the per-list mid-range centre, half range, scale and (zeroed) radius, the blocked int8 copy of the residuals + per-row
// |xi|^2 and residual bound + the per-list radius, and the per-batch images of the (query, probed list) pairs
hipError_t launch_list_minmax(const float *rows, const uint64_t *list_off, uint32_t n_clusters, uint64_t max_list_len, uint32_t dim,
                              uint32_t *kmin, uint32_t *kmax, hipStream_t s, const uint32_t *row_of = nullptr);
hipError_t launch_list_center(const uint32_t *kmin, const uint32_t *kmax, uint32_t n_clusters, uint32_t dim, const uint64_t *list_off,
                              float *center, float *half, float *scale, float *radius, hipStream_t s);
hipError_t launch_global_center(const uint32_t *kmin, const uint32_t *kmax, uint32_t n_clusters, uint32_t dim, const uint64_t *list_off,
                                float *g_center, float *g_half_scale, hipStream_t s);
hipError_t launch_broadcast_center(const float *g_center, const float *g_half_scale, uint32_t n_clusters, uint32_t dim, float *center,
                                   float *half, float *scale, hipStream_t s);
hipError_t launch_block_rows_i8(const float *src, const uint64_t *list_off, const uint64_t *blk_off, uint32_t n_clusters,
                                uint64_t max_tiles, uint32_t dim, const float *center, const float *list_scale, const float *list_half,
                                float *list_radius, void *out, int *row_n2i, float *row_res, hipStream_t s, const uint32_t *row_of = nullptr);
hipError_t launch_quantize_pairs_i8(const float *queries, const uint32_t *probe, const float *center, const float *scale, const float *half,
                                    const float *radius, uint32_t n_pairs, uint32_t nprobe, uint32_t dim, void *q_i8, int *q_n2i,
                                    float *q_res, float *q_resu, float *pair_lb, hipStream_t s, const uint32_t *rank_limit = nullptr);
// (rank_limit, with `probe`: optional [n_pairs / nprobe] -- no image for a pair at or beyond its query's limit, pqv_topk_depth)

// k-means++ round with an int8 screen (kernels_build.hip: minupd_screen_kernel; index.rs:354-369): min_d[r] = min(min_d[r],
// d2(row r, row `pick`)) in the reference's order -- but a row's exact distance is evaluated only if a rigorous lower bound
// of it does not exceed min_d[r]: |x - c| >= |xi - ci| / S - rx - rc on int8 images of (row - centre) S (the searcher's residual
// images with ONE list holding the whole subset: launch_list_minmax / launch_list_center / launch_block_rows_i8), |xi - ci|^2 exact
// in int32 from one v_mfma_i32_16x16x64_i8 chain.  After the first dozen rounds a few rows in a hundred are evaluated, and the
// pass reads one byte per value instead of four -- 38 MB for C3's 50 000 x 768 subset, which the L2s keep between rounds.
struct MinUpdScreenArgs {
    const float  *rows;      // [n, dim] f32 (exact evaluations), dim % 64 == 0
    const float4 *img;       // blocked int8 images: 16-row tiles, tile T column cc (16 dims) row j at 16-byte index (T dim/16 + cc) 16 + j
    const int    *n2i;       // [n] |xi|^2
    const float  *res;       // [n] >= |x - centre - xi / S|
    uint64_t      n, pick;
    uint32_t      dim;
    float         inv_s;     // 1 / S
    float         cm;
    float        *min_d;     // [n]
    float        *mirror;    // optional pinned mirror of min_d (see StreamArgs::mirror_f32)
    float        *mirror_t;  // optional chunk-transposed mirror (StreamArgs::mirror_t)
    uint32_t      mirror_chunk, mirror_stride;
    const unsigned long long *pick_dev;   // optional: the pick is read from device memory (the rounds enqueued ahead, kernels_kpp.hip)
    const uint32_t *stop;                 // optional: a non-zero word makes the launch return at once (KppPickArgs::state)
};
hipError_t launch_minupd_screen(const MinUpdScreenArgs &a, hipStream_t s);

// The k-means++ pick of one round on the device (kernels_kpp.hip; index.rs:354-390): total = the worker chunks' sequential f32 sums joined in
// order, threshold = u[round] * total, picks[round] = the first slot whose sequential f32 cumulative sum reaches it -- bit for bit the
// host walk's result.  n <= 57 344, n_chunks <= 1024.  All scratch words start zeroed and carry the round number as a tag.
struct KppPickArgs {
    const float *md;                 // [n] the current minima
    uint32_t n;
    uint32_t chunk, n_chunks;        // worker chunks: chunk c = [c chunk, min(n, (c + 1) chunk))
    unsigned long long *chunk_sum;   // [n_chunks]
    unsigned long long *blk_sum;     // [64]
    unsigned long long *run_sum;     // [4096] pairs of the quarter runs
    unsigned long long *blk_done;    // [64]
    unsigned long long *head;        // [72] the head block's run starts [64] and its last value
    const float *u;                  // [k] gen_range(0.0..1.0) draws by round
    uint32_t round;                  // 1 .. k - 1
    unsigned long long *picks;       // [k] picks[round] is written
    unsigned long long *stamps;      // optional [32]: diagnostics (pqv_kpp_pick with PQV_KPP_STAMPS=1)
    uint32_t *state;                 // [0] != 0: stopped; [1] the round the host has to decide; [2] why (1 total, 2 value, 3 no slot, 4 wait, 5 slot); [3] bits of the last total
};
hipError_t launch_kpp_pick(const KppPickArgs &a, hipStream_t s);

// out[i, :] = src[idx[i], :]  (sampling gather and the IVF-order re-layout)
hipError_t launch_gather_rows(const float *src, const uint32_t *idx32, const uint64_t *idx64,
                              uint64_t m, uint32_t dim, float *out, hipStream_t s);
// out[i, :dim_p] = src[idx32 ? idx32[i] : i, :dim] zero-padded (dim, dim_p multiples of 4): see pad_rows_kernel
hipError_t launch_pad_rows(const float *src, const uint32_t *idx32, uint64_t m, uint32_t dim, uint32_t dim_p, float *out, hipStream_t s);
// PQV_COSINE: dst[dst_row ? dst_row[i] : i, :dim] = n(src[i * src_stride, :dim]) (every value times 1 / sqrt of the row's 4-grouped
// squared-norm chain; 0 for a zero row): see normalize_rows_kernel.  dst rows are dim wide.
hipError_t launch_normalize_rows(const float *src, uint32_t src_stride, const uint32_t *dst_row, uint64_t m, uint32_t dim, float *dst,
                                 hipStream_t s);
// f64 -> f32 narrowing of a staged column chunk
hipError_t launch_narrow_f64(const double *src, uint64_t count, float *out, hipStream_t s);

// Lloyd / final assignment: cluster[r] = argmin_j d2(row r, centroid j), strict '<' in
// ascending j.  prev (optional) -> *changed += (prev[r] != cluster[r]); sizes (optional,
// zeroed by the caller) += histogram.
hipError_t launch_assign(const float *rows, uint64_t n, uint32_t dim, const float *centroids,
                         uint32_t k, uint32_t *cluster, const uint32_t *prev,
                         unsigned long long *changed, unsigned long long *sizes,
                         hipStream_t s);

// Lloyd update in reference order: centroid[c][j] = (sum over the cluster's rows in
// ascending row order of x[r][j]) / size, empty clusters stay 0.
hipError_t launch_lloyd_update(const float *rows, uint32_t dim, const uint32_t *list_rows,
                               const uint64_t *list_off, uint32_t k, float *centroids,
                               hipStream_t s);

// ---- range search: per-query segments of hits, sorted by (d2, position) and written out (kernels_range.hip) ----------
// Segments of up to RANGE_SMALL hits are sorted by one block in LDS and written out by it; longer ones are sorted in
// RANGE_SMALL-key tiles, merged pairwise (merge path) between the segment buffer and a compact second buffer, and written out.
constexpr uint32_t RANGE_SMALL = 4096;
struct RangeSeg {                 // a segment of the long-segment path
    uint32_t q;                   // query of the sub-batch
    uint32_t n;                   // hits
    uint64_t alt_off;             // its offset in the second buffer
};
struct RangeSortArgs {
    uint32_t        nq;
    const uint32_t *hit_cnt;      // [nq]
    uint64_t       *keys;         // [nq * seg_stride] (StreamArgs::hit_keys)
    uint32_t       *vals;
    uint64_t        seg_stride;
    const uint64_t *seg_off;      // optional [nq]: packed segments (StreamArgs::seg_off); nullptr: q * seg_stride
    uint64_t       *alt_keys;     // second buffer of the long segments, RangeSeg::alt_off
    uint32_t       *alt_vals;
    const RangeSeg *segs;         // [n_segs] long segments
    uint32_t        n_segs;
    uint64_t        max_results;  // 0: every hit
    const uint64_t *out_off;      // [nq] first output entry of each query
    const uint32_t *ids;          // storage row -> file row id (nullptr => identity)
    int             sqrt_out;     // as MergeArgs::sqrt_out
    uint32_t       *out_rows;
    float          *out_dist;
};
// segments with 0 < n <= RANGE_SMALL: sort and write out (one block per query)
hipError_t launch_range_sort_small(const RangeSortArgs &a, hipStream_t s);
// long segments: sort, merge and write out; max_n = the longest of them (several launches)
hipError_t launch_range_sort_large(const RangeSortArgs &a, uint32_t max_n, uint32_t *launches, hipStream_t s);

// number of per-wave partial lists per (query, probed list)
inline uint32_t waves_per_block() { return 4; }

#ifdef PQV_STAMPS
hipError_t stamps_io(unsigned long long *out, int reset);
#endif
// one per kernel unit: an empty launch -- the runtime loads the unit's code object (api.cpp: use_device, once per device) and sets up
// the stream's hardware queue (a corpus' own stream, when it is made)
hipError_t touch_probe(hipStream_t s);
hipError_t touch_screen(hipStream_t s);
hipError_t touch_brute(hipStream_t s);
hipError_t touch_build(hipStream_t s);
hipError_t touch_layout(hipStream_t s);
hipError_t touch_list(hipStream_t s);
hipError_t touch_kpp(hipStream_t s);
hipError_t touch_range(hipStream_t s);
hipError_t touch_mask(hipStream_t s);
hipError_t touch_predicate(hipStream_t s);
hipError_t touch_partition_range(hipStream_t s);

}  // namespace pqv
