// kernels_half_mask.hip -- the exact row-masked distance pass over a corpus of IEEE binary16 rows (pqv.h: half-precision corpora,
// "masked": pqv_topk_masked_f16, pqv_topk_masked_device_f16, pqv_range_search_masked_f16): masked_stream_h_kernel, the sibling of
// masked_stream_kernel (kernels_mask.hip) for 2-byte rows.
//
// The walk is masked_stream_kernel's -- stream_walk.hpp's filtered walk over the mask's position-indexed bitset, the allowed
// positions of a wave's range compacted into 64-row tiles, positions at or beyond the candidate cap dropped BEFORE the mask is
// looked at -- and the distance of a tile is stream_h_kernel's (chain_tile_h: 16-byte loads of eight halves, hardware widening,
// both 4-group partials of a load parked in the chain tile).  So every key is bit-identical to masked_stream_kernel's over an f32
// corpus that holds the widened values, a row the mask excludes is never loaded, and no load reaches behind a row's last byte.
// The merge and range-sort kernels behind it read keys and storage rows only and follow it untouched.
#include "half_tile.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// masked_stream_h_kernel: grid = (blocks_per_list, nprobe | nj, nq), 4 independent waves per block; modes STREAM_TOPK (per-wave
// lists through WaveTopk) and STREAM_RANGE (hit segments through emit_range_hit).  Rows come from a.mat_h.  The window queue's
// compaction goes through the first 128 words of the wave's chain tile, idle between two tiles: no LDS beside the tile.
// Statistics as masked_stream_kernel: every wave adds the rows it evaluated to embeddings_fetched, the (0, 0) block of a query
// adds n_cand[q] to candidate_rows.
// ------------------------------------------------------------------------------------
template <int CGH, int S, int MODE, bool SEQ, int ALIGN>
__global__ __launch_bounds__(256) void masked_stream_h_kernel(const StreamArgs a, const MaskedArgs ma) {
    static_assert(tile_words_h<CGH, SEQ>() >= WindowQueue<false>::SCRATCH, "the compaction needs 128 words of the tile area");
    __shared__ float lds_all[4 * tile_words_h<CGH, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words_h<CGH, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y + (MODE == STREAM_RANGE ? a.j0 : 0u);
    const WalkRange w = walk_range<true>(a, q, j, wave);
    unsigned long long *st = stats_slot(ma.stats, q);
    stats_add_candidates(st, ma.n_cand, q, j);
    const float *qv = a.queries + (uint64_t)q * a.dim;

    WaveTopk<S> tk;
    if constexpr (MODE == STREAM_TOPK) tk.init();

    const uint32_t n_eval = filtered_walk<false>(
        w.lbeg, w.r0, w.r1, lds, lane,
        [&](uint64_t p, uint64_t, uint64_t, uint32_t &) { return image_window(ma.bits, p); },
        [&](const QueueTile &t) {
            const uint32_t my_srow = storage_row(a, w.lbeg + t.my_r);
            const float sum = chain_tile_h<CGH, SEQ, ALIGN>(a, lds, qv, my_srow, t.nvalid, lane);
            const uint64_t pos = w.cbase + t.my_r;
            const bool valid = (uint32_t)lane < t.nvalid;           // (pos < lim by the clamp of the walk)
            if constexpr (MODE == STREAM_TOPK) tk.offer(valid ? l2_key(sum, pos) : KEY_EMPTY, my_srow, a.k, lane);
            else emit_l2_range_hit(a, q, valid, sum, pos, my_srow, lane);
        });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    if constexpr (MODE == STREAM_TOPK) write_partial_lists<S>(a.part_keys, a.part_vals, partial_base(a, q, j, wave, a.k), a.k, lane, tk.key, tk.val);
}

// The chunk choice and the load form are launch_stream_h's: PQV_L2SQ_SEQ -> CGH 8; rows of at most 128 dims -> CGH 16; else CGH 32;
// 16-byte loads where dim % 8 == 0, dwords where dim is even, else halves.
template <int S, int MODE>
static hipError_t launch_masked_stream_h_s(const StreamArgs &a, const MaskedArgs &ma, hipStream_t s) {
    const dim3 grid(a.blocks_per_list, MODE == STREAM_RANGE ? a.nj : a.nprobe, a.nq);
    auto go = [&](auto cgh, auto seq, auto align) {
        hipLaunchKernelGGL((masked_stream_h_kernel<cgh.value, S, MODE, seq.value, align.value>), grid, dim3(256), 0, s, a, ma);
        return hipGetLastError();
    };
    auto by_align = [&](auto cgh, auto seq) {
        if (a.dim % 8 == 0) return go(cgh, seq, std::integral_constant<int, 16>{});
        if (a.dim % 2 == 0) return go(cgh, seq, std::integral_constant<int, 4>{});
        return go(cgh, seq, std::integral_constant<int, 2>{});
    };
    if (a.metric == 1) return by_align(std::integral_constant<int, 8>{}, std::true_type{});
    if (a.dim <= 128) return by_align(std::integral_constant<int, 16>{}, std::false_type{});
    return by_align(std::integral_constant<int, 32>{}, std::false_type{});
}

hipError_t launch_masked_stream_h(const StreamArgs &a, const MaskedArgs &ma, StreamMode mode, hipStream_t s) {
    if (!a.mat_h || !ma.bits || ma.rank_limit || !a.probe || !a.list_off || !a.cand_base || (a.metric != 0 && a.metric != 1)) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0) return hipSuccess;
    if (mode == STREAM_RANGE) return a.nj == 0 ? hipSuccess : launch_masked_stream_h_s<1, STREAM_RANGE>(a, ma, s);
    if (mode != STREAM_TOPK) return hipErrorInvalidValue;
    if (a.nprobe == 0) return hipSuccess;
    return dispatch_list_slots(a.k, [&](auto slots) { return launch_masked_stream_h_s<slots.value, STREAM_TOPK>(a, ma, s); });
}

}  // namespace pqv
