// kernels_distinct.hip -- gfx950 kernels of the distinct top-k (pqv.h: pqv_topk_distinct): the nearest row of each of the k nearest
// groups, a group being the considered rows of one value of a key column (pqv_row_keys).
//
//   WaveDistinctTopk<S, GW>   WaveTopk's wave-distributed ascending list plus each entry's group value, at most ONE entry per group
//   distinct_stream_kernel    masked_stream_kernel's exact walk (kernels_mask.hip) offering (key, storage row, group) to that list
//   distinct_merge_kernel     one wave per query folds the per-wave partial lists through the same offer and writes the result
//
// Why nothing of the plain top-k is reused behind the distance chain: WaveTopk's admission threshold, merge_kernel's pre-filter
// cut and merge_select_large's radix select are all "k-th smallest KEY" bounds, and with several rows per group the k-th smallest
// key is no bound on the k-th GROUP.  The only bound used here is the k-th entry of a list that is already distinct.
//
// The invariant (tests/test_distinct_host.py models it): after any sequence of offers the first k entries of the list are the k
// smallest group representatives of everything offered.  A candidate x of group g is refused only when x >= kth(k) at that moment
// or when g's entry in the list is smaller than x.  kth(k) never increases -- an insert shifts entries up by one from the rank of
// x, a replace shifts only the span between the rank of x and g's old entry -- so a refused candidate stays at or above the final
// k-th entry: it either is not the best row of its group, or its group is not among the k nearest.
//
// The fold is exact for the same reason the plain one is: partial lists are sorted and internally distinct, and a group that is
// in the global top k is, with its global representative r, in the top k of the partition P that holds r -- every group that
// precedes it in P's list has a representative in P smaller than r, hence a global representative smaller than r, and fewer than
// k groups have one.  So r reaches the fold, where the same offer keeps the smallest entry per group.
#include "stream_walk.hpp"
#include "wave_group_lists.hpp"

namespace pqv {

// WaveDistinctTopk<S, GW>: wave_group_lists.hpp

// ------------------------------------------------------------------------------------
// distinct_stream_kernel
//
// masked_stream_kernel's STREAM_TOPK pass, composed of the same pieces (stream_walk.hpp): its grid (row block, probe rank, query),
// its 4 independent waves per block, its clamped walk range, its filtered walk, its chain tile, its keys
// (d2 bits << 32) | (u32)(cbase + position) and its statistics words.  A window's 64
// bits are the funnel-shifted words of the group column's validity image ANDed with those of the shared mask -- all ones where the
// call has neither -- clipped to the range and the cap exactly as there: a NULL-key row belongs to no group and is never read.
// What is new: lane l loads its row's group value key_pos[lbeg + my_r] (one gathered 4- / 8-byte load per evaluated row, issued
// ahead of the chain) and offers (key, storage row, group) to a WaveDistinctTopk.  The wave's list goes to part_keys / part_vals /
// part_grp [nq][n_part][k], group values widened to i64.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
__global__ __launch_bounds__(256) void distinct_stream_kernel(const StreamArgs a, const DistinctArgs da) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<false>::SCRATCH, "the compaction needs 128 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y;
    // a rank at or beyond the query's limit (pqv_topk_distinct_expand) walks nothing: that one word is all the block loads
    if (da.rank_limit && j >= da.rank_limit[q]) {
        write_empty_distinct_list(a, da.part_grp, partial_base(a, q, j, wave, a.k), lane);
        return;
    }
    const WalkRange w = walk_range<true>(a, q, j, wave);
    unsigned long long *st = stats_slot(da.stats, q);
    stats_add_candidates(st, da.n_cand, q, j);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveDistinctTopk<S, GW> tk;
    tk.init();

    const uint32_t n_eval = filtered_walk<false>(
        w.lbeg, w.r0, w.r1, lds, lane,
        [&](uint64_t p, uint64_t, uint64_t clip, uint32_t &) { return group_images_window(da.valid_pos, da.bits, p, clip); },
        [&](const QueueTile &t) { distinct_tile<CG, SEQ, ALIGNED, GW>(a, da.key_pos, w, t, lds, qv, lane, tk); });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
    write_distinct_lists<S, GW>(a, da.part_grp, partial_base(a, q, j, wave, a.k), lane, tk);
}

template <int S, int GW>
static hipError_t launch_distinct_s(const StreamArgs &a, const DistinctArgs &da, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
        hipLaunchKernelGGL((distinct_stream_kernel<cg.value, S, seq.value, aligned.value, GW>), grid, dim3(256), 0, s, a, da);
        return hipGetLastError();
    });
}

template <int GW>
static hipError_t launch_distinct_w(const StreamArgs &a, const DistinctArgs &da, hipStream_t s) {
    return dispatch_list_slots(a.k, [&](auto S) { return launch_distinct_s<S.value, GW>(a, da, s); });
}

hipError_t launch_distinct_stream(const StreamArgs &a, const DistinctArgs &da, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base || !a.part_keys || !a.part_vals) return hipErrorInvalidValue;
    if (!da.key_pos || !da.part_grp || a.k == 0) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0 || a.nprobe == 0) return hipSuccess;
    if (da.elem_size == 4) return launch_distinct_w<1>(a, da, s);
    if (da.elem_size == 8) return launch_distinct_w<2>(a, da, s);
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------
// distinct_merge_kernel: one wave per query folds the query's n_part partial lists through WaveDistinctTopk::offer, 64 entries of
// a list per step and four steps' loads in flight.  No cut, pre-filter or select over the undeduplicated keys: a step is skipped
// only when none of its keys is below the list's current k-th entry (inside offer).  Then the write-out: storage row -> reported
// row through ids, sqrt (IEEE) or the cosine halving, the group value as i64, n_found, and the padding behind it (0xFFFFFFFF,
// +inf, 0).  No tie flag: the order is (d2, position) always.
// ------------------------------------------------------------------------------------
template <int S, int GW>
__global__ __launch_bounds__(64) void distinct_merge_kernel(const DistinctMergeArgs a) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint32_t k = a.k;
    WaveDistinctTopk<S, GW> tk;
    tk.init();

    const uint32_t nchunk = (k + 63) / 64;                     // 64-entry steps per partial list
    const uint64_t n_items = (uint64_t)a.n_part * nchunk;
    const uint64_t qbase = (uint64_t)q * a.n_part * k;
    constexpr int NU = 4;
    for (uint64_t i0 = 0; i0 < n_items; i0 += NU) {
        uint64_t kv[NU];
        uint32_t vv[NU];
        uint32_t gv[NU][GW];
#pragma unroll
        for (int u = 0; u < NU; ++u) {
            const uint64_t i = i0 + u;
            const uint32_t e = (uint32_t)(i % nchunk) * 64 + (uint32_t)lane;
            const bool in = i < n_items && e < k;
            const uint64_t o = qbase + (i / nchunk) * k + e;
            kv[u] = in ? a.part_keys[o] : KEY_EMPTY;
            vv[u] = in ? a.part_vals[o] : 0xFFFFFFFFu;
            const uint64_t g = in ? (uint64_t)a.part_grp[o] : 0ull;
            gv[u][0] = (uint32_t)g;
            if constexpr (GW == 2) gv[u][1] = (uint32_t)(g >> 32);
        }
#pragma unroll
        for (int u = 0; u < NU; ++u) tk.offer(kv[u], vv[u], gv[u], k, lane);
    }

    uint32_t found = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        const bool have = e < k && tk.key[s] != KEY_EMPTY;
        found += (uint32_t)__popcll(__ballot(have));
        if (e < k) {
            uint32_t row = 0xFFFFFFFFu;
            float d = INFINITY;
            int64_t g = 0;
            if (have) {
                const float d2 = __uint_as_float((uint32_t)(tk.key[s] >> 32));
                row = a.ids ? a.ids[tk.val[s]] : tk.val[s];
                d = a.sqrt_out == 1 ? sqrt_f32_ieee(d2) : a.sqrt_out == 2 ? 0.5f * d2 : d2;
                if constexpr (GW == 1) g = (int64_t)(int32_t)tk.grp[s][0];
                else g = (int64_t)(((uint64_t)tk.grp[s][1] << 32) | (uint64_t)tk.grp[s][0]);
            }
            const uint64_t o = (uint64_t)q * k + e;
            a.row_idx[o] = row;
            a.dist[o] = d;
            if (a.group_key) a.group_key[o] = g;
        }
    }
    if (a.n_found && lane == 0) a.n_found[q] = found;
}

hipError_t launch_distinct_merge(const DistinctMergeArgs &a, hipStream_t s) {
    if (!a.part_keys || !a.part_vals || !a.part_grp || !a.row_idx || !a.dist || a.k == 0) return hipErrorInvalidValue;
    if (a.elem_size != 4 && a.elem_size != 8) return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    const dim3 grid(a.nq), block(64);
    const bool w = a.elem_size == 8;
    return dispatch_list_slots(a.k, [&](auto S) {
        if (w) hipLaunchKernelGGL((distinct_merge_kernel<S.value, 2>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((distinct_merge_kernel<S.value, 1>), grid, block, 0, s, a);
        return hipGetLastError();
    });
}

}  // namespace pqv
