// kernels_distinct_filter.hip -- gfx950 kernels of the distinct and grouped top-k under a PER-QUERY key filter (pqv.h:
// pqv_topk_distinct_filtered, pqv_topk_grouped_filtered): every query of a batch has its own tenant, key set or key range, and
// gets documents back.
//
//   distinct_filter_stream_kernel   distinct_stream_kernel's walk (kernels_distinct.hip) over the positions that pass the query's filter
//   grouped_filter_stream_kernel    grouped_stream_kernel's walk (kernels_grouped.hip), pass 2, over the same positions
//
// Both offer to the twins' lists (wave_group_lists.hpp) and write the twins' partial-list formats, so distinct_merge_kernel,
// group_set_kernel and grouped_merge_kernel fold them unchanged.  The contract is equality with the twin under the shared mask
// M_q = filter validity AND F_q(filter key) AND shared mask: a window here has exactly the bits the twin's window has under M_q, so
// the queue, the tiles, the chain and the offers are the twin's.
//
// The filter window, as masked_stream_kernel forms it for WIN 1 - 6 (kernels_mask.hip): lane l loads filter_key_pos[p + l] (one
// coalesced 256- / 512-byte read per window; the column is padded by a whole window), widens an i32 value, and the __ballot of the
// query's test is the window.  It is ANDed with the funnel-shifted words of the filter column's validity image, the group column's
// validity image and the shared mask's image.  The images come first: a window none of whose positions they allow reads no key.
//
// What is compiled: the filter column's width and the group column's width (grouped) are wave-uniform runtime branches around
// the one load; PQV_KEY_EQ runs as the range [a[q], a[q]], so EQ and RANGE are ONE test (lo <= key && key <= hi, two wave-uniform
// scalars loaded once).  Only PQV_KEY_IN is a template flag: it alone has the 8 KiB LDS copy of the query's slice and the block's
// one barrier, which every wave reaches before it looks at its range.  So the distinct form has the twin's 30 instantiations x 2
// and the grouped form -- whose list does not depend on the group column's width -- 15 x 2.
#include "stream_walk.hpp"
#include "wave_group_lists.hpp"

namespace pqv {

// group_filter_bounds: stream_walk.hpp

// ------------------------------------------------------------------------------------
// distinct_filter_stream_kernel
//
// distinct_stream_kernel with one more source of a window's bits; everything else is the twin's, from the same pieces
// (stream_walk.hpp): the walk range clamped at the cap BEFORE any filter, the filtered walk, distinct_tile, the statistics words,
// and part_keys / part_vals / part_grp [nq][n_part][k].
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW, bool IN>
__global__ __launch_bounds__(256) void distinct_filter_stream_kernel(const StreamArgs a, const DistinctArgs da, const GroupFilterArgs fa) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<false>::SCRATCH, "the compaction needs 128 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y;
    // a rank at or beyond the query's limit (pqv_topk_distinct_expand) walks nothing (block-uniform: nobody is left at the barrier)
    if (da.rank_limit && j >= da.rank_limit[q]) {
        write_empty_distinct_list(a, da.part_grp, partial_base(a, q, j, wave, a.k), lane);
        return;
    }
    // the query's test (block-uniform; IN: every wave of the block passes the barrier before it looks at its range)
    KeyTest<IN ? 2 : 1> kt;
    if constexpr (IN) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        kt.setup_in(fa.a, fa.b, q, set_lds);
    } else {
        group_filter_bounds(fa, q, kt);
    }

    WalkRange w = walk_range<true>(a, q, j, wave);
    if (kt.empty()) w.r1 = 0;           // (nothing matches: no window is read)
    unsigned long long *st = stats_slot(da.stats, q);
    stats_add_candidates(st, da.n_cand, q, j);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveDistinctTopk<S, GW> tk;
    tk.init();

    const uint32_t n_eval = filtered_walk<false>(
        w.lbeg, w.r0, w.r1, lds, lane,
        [&](uint64_t p, uint64_t, uint64_t clip, uint32_t &) {
            const uint64_t win = group_images_window(da.valid_pos, da.bits, p, clip);
            if (win == 0) return win;
            return win & kt.window(fa.key_pos, fa.elem_size == 4, fa.valid_pos, p, lane);
        },
        [&](const QueueTile &t) { distinct_tile<CG, SEQ, ALIGNED, GW>(a, da.key_pos, w, t, lds, qv, lane, tk); });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
    write_distinct_lists<S, GW>(a, da.part_grp, partial_base(a, q, j, wave, a.k), lane, tk);
}

template <int S, int GW>
static hipError_t launch_distinct_filter_s(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
        if (fa.kind == 2) hipLaunchKernelGGL((distinct_filter_stream_kernel<cg.value, S, seq.value, aligned.value, GW, true>), grid, dim3(256), 0, s, a, da, fa);
        else hipLaunchKernelGGL((distinct_filter_stream_kernel<cg.value, S, seq.value, aligned.value, GW, false>), grid, dim3(256), 0, s, a, da, fa);
        return hipGetLastError();
    });
}

template <int GW>
static hipError_t launch_distinct_filter_w(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s) {
    return dispatch_list_slots(a.k, [&](auto S) { return launch_distinct_filter_s<S.value, GW>(a, da, fa, s); });
}

static bool group_filter_args_ok(const GroupFilterArgs &fa) {
    if (!fa.key_pos || !fa.a || fa.kind > 2 || (fa.kind != 0 && !fa.b)) return false;
    return fa.elem_size == 4 || fa.elem_size == 8;
}

hipError_t launch_distinct_filter_stream(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base || !a.part_keys || !a.part_vals) return hipErrorInvalidValue;
    if (!da.key_pos || !da.part_grp || a.k == 0) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0 || a.nprobe == 0) return hipSuccess;
    if (!group_filter_args_ok(fa)) return hipErrorInvalidValue;
    if (da.elem_size == 4) return launch_distinct_filter_w<1>(a, da, fa, s);
    if (da.elem_size == 8) return launch_distinct_filter_w<2>(a, da, fa, s);
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------
// grouped_filter_stream_kernel
//
// grouped_stream_kernel (pass 2) with one more source of a window's bits: the group column's validity image, the shared mask's
// image, the query's filter, and membership in the k groups pass 1 named -- in that order, each skipped when nothing is left.  The
// sorted set (5 KB) is staged beside the tile area as there, an IN slice (8 KiB) behind it, both ahead of the block's barrier.  The
// group column's width is a wave-uniform branch around the membership load: WaveGroupedTopk does not depend on it.  Outputs:
// part_keys / part_vals / part_slot [nq][n_part][km] and part_cnt [nq][n_part], the rows evaluated added to embeddings_fetched.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, bool IN>
__global__ __launch_bounds__(256) void grouped_filter_stream_kernel(const StreamArgs a, const GroupedArgs ga, const GroupFilterArgs fa) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    __shared__ int64_t set_v[GROUPED_SET_MAX];
    __shared__ uint16_t set_s[GROUPED_SET_MAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y;
    // a rank at or beyond the query's limit (pqv_topk_grouped_expand) walks nothing (block-uniform: nobody is left at the barrier)
    if (ga.rank_limit && j >= ga.rank_limit[q]) {
        if (lane == 0) ga.part_cnt[partial_base(a, q, j, wave, 1)] = 0;
        return;
    }
    // the query's set and test (block-uniform; every wave of the block passes the barrier before it looks at its range)
    GroupSet gs;
    gs.stage(ga, q, set_v, set_s);
    KeyTest<IN ? 2 : 1> kt;
    if constexpr (IN) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        kt.setup_in(fa.a, fa.b, q, set_lds);        // (its barrier covers set_v / set_s too)
    } else {
        group_filter_bounds(fa, q, kt);
        __syncthreads();
    }

    WalkRange w = walk_range<true>(a, q, j, wave);
    if (gs.n == 0) w.r1 = 0;            // no group: nothing to walk, an empty list is written
    if (kt.empty()) w.r1 = 0;           // (cannot be with groups: a group of pass 1 has a passing row)
    unsigned long long *st = stats_slot(ga.stats, q);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveGroupedTopk<S> tk;
    tk.init();

    const uint32_t n_eval = filtered_walk<true>(
        w.lbeg, w.r0, w.r1, lds, lane,
        [&](uint64_t p, uint64_t, uint64_t clip, uint32_t &slot) {
            uint64_t win = group_images_window(ga.valid_pos, ga.bits, p, clip);
            if (win == 0) return win;
            win &= kt.window(fa.key_pos, fa.elem_size == 4, fa.valid_pos, p, lane);
            if (win == 0) return win;
            return win & group_member_window(gs, ga.key_pos, ga.elem_size == 4, p, lane, slot);
        },
        [&](const QueueTile &t) { grouped_tile<CG, SEQ, ALIGNED>(a, ga.group_size, w, t, lds, qv, lane, tk); });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
    write_grouped_lists<S>(a, ga, q, j, wave, lane, tk);
}

template <int S>
static hipError_t launch_grouped_filter_s(const StreamArgs &a, const GroupedArgs &ga, const GroupFilterArgs &fa, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
        if (fa.kind == 2) hipLaunchKernelGGL((grouped_filter_stream_kernel<cg.value, S, seq.value, aligned.value, true>), grid, dim3(256), 0, s, a, ga, fa);
        else hipLaunchKernelGGL((grouped_filter_stream_kernel<cg.value, S, seq.value, aligned.value, false>), grid, dim3(256), 0, s, a, ga, fa);
        return hipGetLastError();
    });
}

hipError_t launch_grouped_filter_stream(const StreamArgs &a, const GroupedArgs &ga, const GroupFilterArgs &fa, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base || !ga.part_keys || !ga.part_vals || !ga.part_slot || !ga.part_cnt) return hipErrorInvalidValue;
    if (!ga.key_pos || !ga.set_keys || !ga.set_slot || !ga.n_found) return hipErrorInvalidValue;
    // k * group_size <= 1024 with group_size >= 2 (one row per group is the distinct call), hence k <= GROUPED_SET_MAX
    if (ga.k == 0 || ga.group_size < 2 || (uint64_t)ga.k * ga.group_size != ga.km || ga.km > 1024 || ga.k > GROUPED_SET_MAX) return hipErrorInvalidValue;
    if (ga.elem_size != 4 && ga.elem_size != 8) return hipErrorInvalidValue;
    if (!group_filter_args_ok(fa)) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0 || a.nprobe == 0) return hipSuccess;
    return dispatch_list_slots(ga.km, [&](auto S) { return launch_grouped_filter_s<S.value>(a, ga, fa, s); });
}

}  // namespace pqv
