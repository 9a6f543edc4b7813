// kernels_partition_range.hip -- gfx950 kernel of the range search over a key partition (pqv.h: pqv_range_search_partition): every
// considered row of a query's candidate sequence within a radius, appended to the query's hit segment.
//   partition_range_kernel   partition_stream_kernel's walk (PartitionSeq, stream_walk.hpp) with STREAM_RANGE's output
//                            (emit_range_hit) in place of the per-wave top-k lists
// The segments are PACKED: query q's begins at seg_off[q] and holds n_cand[q] entries (the host sizes them from the span kernel's
// counts), so a skewed batch costs the sum of its sequences, not nq times the longest.  kernels_range.hip sorts each segment by
// (distance key, sequence position) -- unique per query, so the answer does not depend on the order the waves appended in or on the
// grid -- and writes it out.
#include "stream_walk.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// partition_range_kernel
//
// grid = (B, queries of the group); block = 256 threads = 4 independent waves with partition_stream_kernel's tile area and nothing
// beside it.  Wave w of block x takes the 64-position windows (turn * B + x) * 4 + w of its query's sequence while they begin
// inside it.  MASKED = false: the window IS the tile.  MASKED: the lanes ballot their positions' bits of the mask's image and the
// set ones are compacted through a WindowQueue with the list position as payload (PartitionSeq::filtered_windows), so a row the
// mask excludes is never loaded; sequence positions stay the unmasked ones.
// Every tile tests out <= radius on the output scale (L2 forms: sqrt_out 0 d2, 1 sqrt(d2), 2 0.5 d2; DOT: dist = 0.0f - s) and
// appends (l2_key / dot_key of the sequence position, storage row): one ballot, an mbcnt rank and one atomicAdd on hit_cnt[q] per
// wave and tile.  A NaN distance never compares true.  hits <= considered rows <= n_cand[q] = the segment's room.
// No per-wave list: no S parameter, nothing written by a wave without a hit.  One statistics add per wave: the rows evaluated.
// ------------------------------------------------------------------------------------
template <int CG, bool SEQ, bool ALIGNED, bool DOT, bool MASKED>
__global__ __launch_bounds__(256) void partition_range_kernel(const StreamArgs a, const PartitionArgs pa) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.y;
    PartitionSeq ps;
    ps.setup(pa, q);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    uint32_t n_eval = 0;

    // a tile of nvalid rows: lane l holds list position lpos at sequence position seq (both clamped to the tile's last row)
    auto tile = [&](uint32_t lpos, uint32_t seq, uint32_t nvalid) {
        const uint32_t my_srow = storage_row(a, lpos);
        const bool valid = (uint32_t)lane < nvalid;
        if constexpr (DOT) {
            const float sum = dot_tile<CG, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
            const float dist = 0.0f - sum;
            emit_range_hit(a, q, valid && dist <= a.radius, dot_key(sum, seq), my_srow, lane);
        } else {
            const float sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
            emit_l2_range_hit(a, q, valid, sum, seq, my_srow, lane);
        }
        n_eval += nvalid;
    };

    if constexpr (!MASKED) {
        ps.windows(ps.total, wave, lane, [&](uint64_t, uint32_t nvalid, uint32_t seq, uint32_t lpos) { tile(lpos, seq, nvalid); });
    } else {
        ps.filtered_windows(ps.total, lds, wave, lane, [&](uint32_t lpos) { return image_bit(pa.bits, lpos); }, tile);
    }
    unsigned long long *st = stats_slot(pa.stats, q);
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
}

template <bool DOT, bool MASKED>
static hipError_t launch_partition_range_m(const StreamArgs &a, const PartitionArgs &pa, hipStream_t s) {
    return dispatch_chunk<!DOT>(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nq);
        hipLaunchKernelGGL((partition_range_kernel<cg.value, seq.value, aligned.value, DOT, MASKED>), grid, dim3(256), 0, s, a, pa);
        return hipGetLastError();
    });
}

hipError_t launch_partition_range(const StreamArgs &a, const PartitionArgs &pa, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!partition_walk_ok(a, pa)) return hipErrorInvalidValue;
    if (!a.hit_cnt || !a.hit_keys || !a.hit_vals || (!a.seg_off && a.seg_stride == 0)) return hipErrorInvalidValue;
    if (a.metric == 4) return pa.bits ? launch_partition_range_m<true, true>(a, pa, s) : launch_partition_range_m<true, false>(a, pa, s);     // PQV_DOT
    return pa.bits ? launch_partition_range_m<false, true>(a, pa, s) : launch_partition_range_m<false, false>(a, pa, s);
}

__global__ void touch_partition_range_kernel() {}
hipError_t touch_partition_range(hipStream_t s) {
    hipLaunchKernelGGL(touch_partition_range_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace pqv
