// kernels_rows.hip -- gfx950 kernels of the candidate-list calls (pqv.h: pqv_topk_rows, pqv_score_rows): exact distances over the
// rows a caller names per query, cand_rows[lims[q] .. lims[q + 1]).
//   row_map_kernel      the searcher's row -> list position map: map[ids[p]] = p over a table filled with ROW_EMPTY
//   rows_stream_kernel  partition_stream_kernel's tile, list and grid over RowsSeq's walk: a sequence position is a candidate's index
//                       in its slice, its entry map[cand_rows[...]]; SCORE: no list -- every candidate's distance goes to its own
//                       slot of the output instead, +inf for the ones that are not walked
// Nothing is probed and nothing is screened: a candidate whose row is in no list, or whose mask bit is clear, is never loaded.
#include "stream_walk.hpp"

namespace pqv {

constexpr uint32_t ROW_EMPTY = 0xFFFFFFFFu;     // a row no list holds (no list position has that value: a searcher has < 2^32 of them)

// (the caller has filled map[0 .. map_len) with ROW_EMPTY on the same stream)
__global__ __launch_bounds__(256) void row_map_kernel(const uint32_t *ids, uint64_t n_pos, uint32_t *map, uint64_t map_len) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (p >= n_pos) return;
    const uint64_t r = ids[p];
    if (r < map_len) map[r] = (uint32_t)p;
}

hipError_t launch_row_map(const uint32_t *ids, uint64_t n_pos, uint32_t *map, uint64_t map_len, hipStream_t s) {
    if (n_pos > 0xFFFFFFFFull || map_len > 0xFFFFFFFFull) return hipErrorInvalidValue;
    if (map_len == 0) return hipSuccess;
    if (!map || (n_pos && !ids)) return hipErrorInvalidValue;
    if (hipError_t e = hipMemsetAsync(map, 0xFF, map_len * sizeof(uint32_t), s)) return e;
    if (n_pos == 0) return hipSuccess;
    hipLaunchKernelGGL(row_map_kernel, dim3((uint32_t)((n_pos + 255) / 256)), dim3(256), 0, s, ids, n_pos, map, map_len);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// A caller-given candidate sequence: PartitionSeq's sibling for walk_seq_windows (stream_walk.hpp).  Query q's sequence is its slice
// of cand_rows as given -- total = min(lims[q + 1] - lims[q], 2^32 - 1) positions, none for an inverted slice -- and entry(seq) is
// two dependent gathered words: the row id, then -- only behind the compare against the map's length -- its list position.  A row
// at or beyond the map, 0xFFFFFFFF included, and a row of no list give ROW_EMPTY.
// ------------------------------------------------------------------------------------
struct RowsSeq {
    uint32_t total;
    uint64_t beg, map_len;
    const uint32_t *rows, *map;

    __device__ __forceinline__ void setup(const RowsArgs &ra, uint32_t q) {
        const uint64_t s0 = uniform_word(ra.lims + q), s1 = uniform_word(ra.lims + q + 1);
        const uint64_t len = s1 > s0 ? s1 - s0 : 0;
        total = len > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)len;
        beg = s0;
        rows = ra.cand_rows; map = ra.map; map_len = ra.map_len;
    }
    __device__ __forceinline__ uint32_t entry(uint32_t seq) const {
        const uint32_t r = rows[beg + seq];
        return r < map_len ? map[r] : ROW_EMPTY;
    }
};

// ------------------------------------------------------------------------------------
// rows_stream_kernel
//
// grid = (B, nq); block = 256 threads = 4 independent waves, partition_stream_kernel's in everything but the sequence: wave w of
// block x takes the 64-position windows (turn * B + x) * 4 + w of the query's slice, and the walk is always the filtered one -- a
// position is walked iff its entry is a list position and image_bit of the mask's image (nullptr: set) holds.  Sequence positions
// stay the slice's own, so keys order by (distance key, index in the slice) and a row listed twice is two candidates.
// !SCORE: the per-wave lists go out in StreamArgs' format (nprobe = 1, blocks_per_list = B) for merge_kernel / dot_merge_kernel.
// SCORE: a.out_f32[lims[q] - *lims0 + seq] = the candidate's distance on the output scale, transformed as the merge kernels'
// write-out transforms a key's (a.sqrt_out 1: IEEE sqrt; 2: halved; DOT: 0.0f - s), or +inf from the window loop where the
// candidate is not walked: every slot is written exactly once, by the lane that owns the position.
// The query's block 0 writes n_cand_out[q] and adds the slice length to candidate_rows; every wave adds the rows it evaluated to
// embeddings_fetched.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, bool DOT, bool SCORE>
__global__ __launch_bounds__(256, (CG == 32 && S <= 4) ? 5 : 1) void rows_stream_kernel(const StreamArgs a, const RowsArgs ra) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.y;
    RowsSeq rs;
    rs.setup(ra, q);
    float *out = nullptr;
    if constexpr (SCORE) {      // (a slice that begins ahead of the call's first one has no place in the output: it is walked as empty)
        const uint64_t l0 = uniform_word(ra.lims0);
        if (rs.beg < l0) rs.total = 0;
        else out = a.out_f32 + (rs.beg - l0);
    }
    unsigned long long *st = stats_slot(ra.stats, q);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (ra.n_cand_out) ra.n_cand_out[q] = rs.total;
        if (st && rs.total) atomicAdd(&st[2], (unsigned long long)rs.total);
    }

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveTopk<S> tk;
    if constexpr (!SCORE) tk.init();
    uint32_t n_eval = 0;

    walk_seq_windows(
        rs.total, lds, wave, lane, [&](uint32_t seq) { return rs.entry(seq); },
        [&](uint32_t lpos, uint32_t seq) {
            const bool on = lpos != ROW_EMPTY && image_bit(ra.bits, lpos);
            if constexpr (SCORE) {
                if (!on) out[seq] = INFINITY;
            }
            return on;
        },
        [&](uint32_t lpos, uint32_t seq, uint32_t nvalid) {
            const uint32_t my_srow = storage_row(a, lpos);
            float sum;
            if constexpr (DOT) sum = dot_tile<CG, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
            else sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
            const bool valid = (uint32_t)lane < nvalid;
            if constexpr (SCORE) {
                float d;
                if constexpr (DOT) d = 0.0f - sum;
                else d = a.sqrt_out == 1 ? sqrt_f32_ieee(sum) : a.sqrt_out == 2 ? 0.5f * sum : sum;
                if (valid) out[seq] = d;
            } else {
                const uint64_t key = DOT ? dot_key(sum, seq) : l2_key(sum, seq);
                tk.offer(valid ? key : KEY_EMPTY, my_srow, a.k, lane);
            }
            n_eval += nvalid;
        });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    if constexpr (!SCORE) write_partial_lists<S>(a.part_keys, a.part_vals, partial_base(a, q, 0, wave, a.k), a.k, lane, tk.key, tk.val);
}

static inline bool rows_walk_ok(const StreamArgs &a, const RowsArgs &ra) {
    if (!ra.lims || (ra.map_len && !ra.map) || ra.map_len > 0xFFFFFFFFull) return false;
    return a.nprobe == 1 && a.blocks_per_list != 0 && a.blocks_per_list <= 0xFFFFu && a.nq <= 0xFFFFu;
}

template <int S, bool DOT, bool SCORE>
static hipError_t launch_rows_s(const StreamArgs &a, const RowsArgs &ra, hipStream_t s) {
    return dispatch_chunk<!DOT>(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nq);
        hipLaunchKernelGGL((rows_stream_kernel<cg.value, S, seq.value, aligned.value, DOT, SCORE>), grid, dim3(256), 0, s, a, ra);
        return hipGetLastError();
    });
}

hipError_t launch_rows_stream(const StreamArgs &a, const RowsArgs &ra, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!rows_walk_ok(a, ra) || !a.part_keys || !a.part_vals) return hipErrorInvalidValue;
    const bool dot = a.metric == 4;     // PQV_DOT
    return dispatch_list_slots(a.k, [&](auto S) {
        return dot ? launch_rows_s<S.value, true, false>(a, ra, s) : launch_rows_s<S.value, false, false>(a, ra, s);
    });
}

hipError_t launch_rows_score(const StreamArgs &a, const RowsArgs &ra, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!rows_walk_ok(a, ra) || !a.out_f32 || !ra.lims0) return hipErrorInvalidValue;
    return a.metric == 4 ? launch_rows_s<1, true, true>(a, ra, s) : launch_rows_s<1, false, true>(a, ra, s);
}

}  // namespace pqv
