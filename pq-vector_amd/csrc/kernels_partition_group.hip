// kernels_partition_group.hip -- gfx950 kernels of the distinct / grouped top-k over a key partition (pqv.h:
// pqv_topk_partition_grouped): the k nearest groups among the rows of a query's candidate sequence, and up to group_size rows of
// each.  The two passes of pqv_topk_grouped (kernels_distinct.hip, kernels_grouped.hip) over partition_stream_kernel's walk
// (kernels_partition.hip), composed of the shared pieces and nothing else:
//
//   partition_distinct_stream_kernel   pass 1: PartitionSeq's windows, the chain tile, WaveDistinctTopk; folded by distinct_merge_kernel
//   partition_grouped_stream_kernel    pass 2: the same windows over the members of the query's GroupSet, WaveGroupedTopk; folded by
//                                      grouped_merge_kernel
//
// A sequence's list positions are scattered (the partition is sorted by key, not by position), so a window's bits are GATHERED:
// lane l tests bit lpos of the mask's image and of the group column's validity image, as partition_stream_kernel's MASKED form tests
// the mask's.  Sequence positions stay the unmasked ones: keys are l2_key(sum, seq), the order is (distance key, position).
#include "stream_walk.hpp"
#include "wave_group_lists.hpp"

namespace pqv {

// the 32-bit words of list position lpos's group value (GW = 1: an i32 column, 2: the halves of an i64): one gathered load
template <int GW>
__device__ __forceinline__ void load_group_words(const void *key_pos, uint32_t lpos, uint32_t (&g)[GW]) {
    if constexpr (GW == 1) {
        g[0] = static_cast<const uint32_t *>(key_pos)[lpos];
    } else {
        const uint64_t gv = static_cast<const uint64_t *>(key_pos)[lpos];
        g[0] = (uint32_t)gv; g[1] = (uint32_t)(gv >> 32);
    }
}

// ------------------------------------------------------------------------------------
// partition_distinct_stream_kernel
//
// partition_stream_kernel's grid (B, nq), its 4 independent waves per block, its windows and its tile area.  FILTERED = false (no
// mask, no validity image): the window IS the tile.  FILTERED: the lanes ballot (mask bit of lpos) && (validity bit of lpos) and
// the set ones are compacted through WindowQueue with lpos as payload; a tile runs per 64 queued positions and once more behind the
// wave's last window, so a masked or NULL-group row is never loaded.  A tile's lane l loads its row's group value key_pos[lpos] (4
// or 8 bytes, gathered, issued ahead of the chain) and offers (key, storage row, group words) to WaveDistinctTopk.  The per-wave
// lists go out as distinct_stream_kernel's do -- part_keys / part_vals / part_grp [nq][B * 4][k] (nprobe = 1, blocks_per_list = B) --
// for distinct_merge_kernel; a wave without a window writes its EMPTY list.  One statistics add per wave: the rows evaluated.
// da.bits / stats / n_cand / rank_limit are not read: the mask and the statistics block are pa's.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW, bool FILTERED>
__global__ __launch_bounds__(256) void partition_distinct_stream_kernel(const StreamArgs a, const PartitionArgs pa, const DistinctArgs da) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.y;
    PartitionSeq ps;
    ps.setup(pa, q);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveDistinctTopk<S, GW> tk;
    tk.init();
    uint32_t n_eval = 0;

    // a tile of nvalid rows: lane l holds list position lpos at sequence position seq (both clamped to the tile's last row)
    auto tile = [&](uint32_t lpos, uint32_t seq, uint32_t nvalid) {
        const uint32_t my_srow = storage_row(a, lpos);
        uint32_t mygrp[GW];
        load_group_words<GW>(da.key_pos, lpos, mygrp);
        const float sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
        const bool valid = (uint32_t)lane < nvalid;
        tk.offer(valid ? l2_key(sum, seq) : KEY_EMPTY, my_srow, mygrp, a.k, lane);
        n_eval += nvalid;
    };

    if constexpr (!FILTERED) {
        ps.windows(ps.total, wave, lane, [&](uint64_t, uint32_t nvalid, uint32_t seq, uint32_t lpos) { tile(lpos, seq, nvalid); });
    } else {
        ps.filtered_windows(ps.total, lds, wave, lane,
                            [&](uint32_t lpos) { return image_bit(pa.bits, lpos) && image_bit(da.valid_pos, lpos); }, tile);
    }
    unsigned long long *st = stats_slot(pa.stats, q);
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    write_distinct_lists<S, GW>(a, da.part_grp, partial_base(a, q, 0, wave, a.k), lane, tk);
}

template <int S, int GW, bool FILTERED>
static hipError_t launch_partition_distinct_s(const StreamArgs &a, const PartitionArgs &pa, const DistinctArgs &da, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nq);
        hipLaunchKernelGGL((partition_distinct_stream_kernel<cg.value, S, seq.value, aligned.value, GW, FILTERED>), grid, dim3(256), 0, s, a, pa, da);
        return hipGetLastError();
    });
}

// what both passes ask beside the walk's arguments (the lists carry L2 keys: no PQV_DOT)
static bool partition_group_walk_ok(const StreamArgs &a, const PartitionArgs &pa) {
    return partition_walk_ok(a, pa) && a.metric != 4 && a.mat && a.queries;
}

hipError_t launch_partition_distinct_stream(const StreamArgs &a, const PartitionArgs &pa, const DistinctArgs &da, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!partition_group_walk_ok(a, pa) || !a.part_keys || !a.part_vals || !da.key_pos || !da.part_grp || a.k == 0) return hipErrorInvalidValue;
    if (da.elem_size != 4 && da.elem_size != 8) return hipErrorInvalidValue;
    const bool filtered = pa.bits || da.valid_pos, wide = da.elem_size == 8;
    return dispatch_list_slots(a.k, [&](auto S) {
        if (wide) return filtered ? launch_partition_distinct_s<S.value, 2, true>(a, pa, da, s) : launch_partition_distinct_s<S.value, 2, false>(a, pa, da, s);
        return filtered ? launch_partition_distinct_s<S.value, 1, true>(a, pa, da, s) : launch_partition_distinct_s<S.value, 1, false>(a, pa, da, s);
    });
}

// ------------------------------------------------------------------------------------
// partition_grouped_stream_kernel
//
// Pass 2: launch_group_set has turned pass 1's group_key / n_found into the query's sorted set.  The block stages it in LDS beside
// the tile area (GroupSet: 5 KiB, as grouped_stream_kernel does) and passes ONE barrier before anything that is not block-uniform.
// A window's bit is mask && validity && membership: lane l looks key_pos[lpos] up in the set.  WindowQueue carries one payload word
// and this kernel needs two (lpos for the row, the slot for the offer): lpos travels, and the tile looks its row's slot up AGAIN --
// one gathered key load and one LDS search per evaluated row, next to a dim-long chain, instead of a wider queue in every filtered
// kernel.  The tile offers (key, storage row, slot) to WaveGroupedTopk; lists and counts go out as write_grouped_lists writes them
// (part_keys / part_vals / part_slot [nq][B * 4][km], part_cnt [nq][B * 4]) for grouped_merge_kernel.  No group (n_found == 0):
// nothing is walked and the count is 0.  ga.bits / stats / rank_limit are not read: the mask and the statistics block are pa's.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
__global__ __launch_bounds__(256) void partition_grouped_stream_kernel(const StreamArgs a, const PartitionArgs pa, const GroupedArgs ga) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    __shared__ int64_t set_v[GROUPED_SET_MAX];
    __shared__ uint16_t set_s[GROUPED_SET_MAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.y;
    // the query's set (block-uniform; every wave of the block passes the barrier before it looks at its windows)
    GroupSet gs;
    gs.stage(ga, q, set_v, set_s);
    __syncthreads();

    PartitionSeq ps;
    ps.setup(pa, q);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveGroupedTopk<S> tk;
    tk.init();
    uint32_t n_eval = 0;

    // a tile of nvalid MEMBERS: lane l holds list position lpos at sequence position seq (both clamped to the tile's last row)
    auto tile = [&](uint32_t lpos, uint32_t seq, uint32_t nvalid) {
        const uint32_t my_srow = storage_row(a, lpos);
        uint32_t slot = 0;
        gs.lookup(load_key_pos(ga.key_pos, GW == 1, lpos), slot);
        const float sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
        const bool valid = (uint32_t)lane < nvalid;
        tk.offer(valid ? l2_key(sum, seq) : KEY_EMPTY, my_srow, slot, ga.group_size, lane);
        n_eval += nvalid;
    };

    // (no group: nothing to walk, an empty list is written)
    ps.filtered_windows(gs.n ? ps.total : 0u, lds, wave, lane,
                        [&](uint32_t lpos) {
                            if (!image_bit(pa.bits, lpos) || !image_bit(ga.valid_pos, lpos)) return false;
                            uint32_t slot = 0;
                            return gs.lookup(load_key_pos(ga.key_pos, GW == 1, lpos), slot);
                        },
                        tile);

    unsigned long long *st = stats_slot(pa.stats, q);
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
    write_grouped_lists<S>(a, ga, q, 0, wave, lane, tk);
}

template <int S, int GW>
static hipError_t launch_partition_grouped_s(const StreamArgs &a, const PartitionArgs &pa, const GroupedArgs &ga, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nq);
        hipLaunchKernelGGL((partition_grouped_stream_kernel<cg.value, S, seq.value, aligned.value, GW>), grid, dim3(256), 0, s, a, pa, ga);
        return hipGetLastError();
    });
}

hipError_t launch_partition_grouped_stream(const StreamArgs &a, const PartitionArgs &pa, const GroupedArgs &ga, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!partition_group_walk_ok(a, pa) || !ga.part_keys || !ga.part_vals || !ga.part_slot || !ga.part_cnt) return hipErrorInvalidValue;
    if (!ga.key_pos || !ga.set_keys || !ga.set_slot || !ga.n_found) return hipErrorInvalidValue;
    // k * group_size == km <= 1024 with group_size >= 2, hence k <= GROUPED_SET_MAX (launch_grouped_stream's shape)
    if (ga.k == 0 || ga.group_size < 2 || (uint64_t)ga.k * ga.group_size != ga.km || ga.km > 1024 || ga.k > GROUPED_SET_MAX) return hipErrorInvalidValue;
    if (ga.elem_size != 4 && ga.elem_size != 8) return hipErrorInvalidValue;
    const bool wide = ga.elem_size == 8;
    return dispatch_list_slots(ga.km, [&](auto S) {
        return wide ? launch_partition_grouped_s<S.value, 2>(a, pa, ga, s) : launch_partition_grouped_s<S.value, 1>(a, pa, ga, s);
    });
}

}  // namespace pqv
