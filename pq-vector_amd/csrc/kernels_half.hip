// kernels_half.hip -- the exact streaming distance pass over a corpus of IEEE binary16 rows (pqv.h: half-precision corpora):
// stream_h_kernel, the sibling of stream_kernel (kernels_probe.hip) for 2-byte rows, and widen_rows_h_kernel (pqv_corpus_fetch_rows).
//
// The distance of a query to an f16 row is DEFINED as the reference chain (index.rs:461-480) over the row widened to f32 -- an
// exact conversion -- so every key this pass writes is bit-identical to stream_kernel's over an f32 corpus that holds the widened
// values.  Grid, walk (walk_range / storage_row), per-wave lists, range hits and outputs are stream_kernel's: the merge and
// range-sort kernels behind it read keys and storage rows, never row values, and follow it untouched.
#include "half_tile.hpp"     // chain_tile_h: the chain tile of 2-byte rows

namespace pqv {

// ------------------------------------------------------------------------------------
// stream_h_kernel: stream_kernel's grid = (blocks_per_list, nprobe | nj, nq), 4 independent waves per block, the same walk and
// the same outputs; modes STREAM_TOPK, STREAM_DIST, STREAM_RANGE.  Rows come from a.mat_h (a.mat is not read).
// ------------------------------------------------------------------------------------
template <int CGH, int S, int MODE, bool SEQ, int ALIGN>
__global__ __launch_bounds__(256) void stream_h_kernel(const StreamArgs a) {
    if (a.zero_u32 && blockIdx.x == 0 && blockIdx.y == 0) {     // scratch the NEXT kernels expect zeroed
        for (uint32_t i = blockIdx.z * 256 + threadIdx.x; i < a.zero_n; i += gridDim.z * 256) a.zero_u32[i] = 0u;
    }
    __shared__ float lds_all[4 * tile_words_h<CGH, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words_h<CGH, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y + (MODE == STREAM_RANGE ? a.j0 : 0u);
    const WalkRange w = walk_range<false>(a, q, j, wave);
    const float *qv = a.queries + (uint64_t)q * a.dim;

    WaveTopk<S> tk;
    if constexpr (MODE == STREAM_TOPK) tk.init();

    for (uint64_t t0 = w.r0; t0 < w.r1; t0 += 64) {
        const uint32_t nvalid = (w.r1 - t0 < 64) ? (uint32_t)(w.r1 - t0) : 64u;
        // storage row of tile row `lane` (clamped so every address is in range)
        const uint32_t lrow = (uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1;
        const uint32_t my_srow = storage_row(a, w.lbeg + t0 + lrow);
        const float sum = chain_tile_h<CGH, SEQ, ALIGN>(a, lds, qv, my_srow, nvalid, lane);

        const uint64_t pos = w.cbase + t0 + (uint64_t)lane;
        const bool valid = (uint32_t)lane < nvalid && pos < w.lim;
        if constexpr (MODE == STREAM_TOPK) {
            tk.offer(valid ? l2_key(sum, pos) : KEY_EMPTY, my_srow, a.k, lane);
        } else if constexpr (MODE == STREAM_RANGE) {
            emit_l2_range_hit(a, q, valid, sum, pos, my_srow, lane);
        } else {
            if (valid) a.out_f32[pos] = sum;
        }
    }

    if constexpr (MODE == STREAM_TOPK) write_partial_lists<S>(a.part_keys, a.part_vals, partial_base(a, q, j, wave, a.k), a.k, lane, tk.key, tk.val);
}

// The chunk choice (the chain order does not depend on it): PQV_L2SQ_SEQ -> CGH 8, eight squares per lane; rows of at most 128
// dims -> CGH 16; else CGH 32.  The load form follows the alignment of the row starts, dim * 2 bytes apart.
template <int S, int MODE>
static hipError_t launch_stream_h_s(const StreamArgs &a, hipStream_t s) {
    const dim3 grid(a.blocks_per_list, MODE == STREAM_RANGE ? a.nj : a.probe ? a.nprobe : 1, a.nq);
    auto go = [&](auto cgh, auto seq, auto align) {
        hipLaunchKernelGGL((stream_h_kernel<cgh.value, S, MODE, seq.value, align.value>), grid, dim3(256), 0, s, a);
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

hipError_t launch_stream_h(const StreamArgs &a, StreamMode mode, hipStream_t s) {
    if (a.nq == 0 || a.blocks_per_list == 0) return hipSuccess;
    if (!a.mat_h || (a.metric != 0 && a.metric != 1)) return hipErrorInvalidValue;
    if (mode == STREAM_RANGE) {
        if (a.nj == 0 || !a.probe) return a.nj == 0 ? hipSuccess : hipErrorInvalidValue;
        return launch_stream_h_s<1, STREAM_RANGE>(a, s);
    }
    if (mode == STREAM_TOPK) {
        return dispatch_list_slots(a.k, [&](auto slots) { return launch_stream_h_s<slots.value, STREAM_TOPK>(a, s); });
    }
    if (mode == STREAM_DIST) return launch_stream_h_s<1, STREAM_DIST>(a, s);
    return hipErrorInvalidValue;
}

// out[i * dim + d] = widen(rows[idx[i] * dim + d]), i < m: pqv_corpus_fetch_rows over an f16 corpus
__global__ __launch_bounds__(256) void widen_rows_h_kernel(const uint16_t *rows, const uint32_t *idx, uint64_t m, uint32_t dim, float *out) {
    const uint64_t total = m * dim;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t r = i / dim;
        out[i] = widen_h(rows[(uint64_t)idx[r] * dim + (i - r * dim)]);
    }
}
hipError_t launch_widen_rows_h(const uint16_t *rows, const uint32_t *idx, uint64_t m, uint32_t dim, float *out, hipStream_t s) {
    if (m == 0) return hipSuccess;
    const uint64_t total = m * dim;
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(widen_rows_h_kernel, dim3(blocks), dim3(256), 0, s, rows, idx, m, dim, out);
    return hipGetLastError();
}

}  // namespace pqv
