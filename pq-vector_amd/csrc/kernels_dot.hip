// kernels_dot.hip -- gfx950 kernels of PQV_DOT (pqv.h): inner-product search.  The distance of a candidate is the negated
// similarity, dist = 0.0f - s(q, x), with s the reference's 4-grouped chain (index.rs:461-480) over PRODUCTS instead of squared
// differences:
//     t_g = ((q0 x0 + q1 x1) + q2 x2) + q3 x3 per full group of four dims, sum += t_g in ascending g, then the dim % 4 tail element
//     by element -- every operation a rounded f32 one (the unit is built with -ffp-contract=off like the others).
// sum starts at +0.0f and x + y is -0.0f only when both are, so sum is never -0.0f and a zero dist is always +0.0f.
// Distances are signed, so the keys are (ord(dist) << 32) | candidate position with ord the usual order-preserving map of f32 bits
// to u32 (negative: all bits flipped; else: the sign bit set): ascending keys = ascending (dist, position).
//   dot_stream_kernel   stream_kernel's grid, tile and chain structure (stream_walk.hpp: dot_tile is chain_tile's products form)
//                       with that key;
//                       WIN = 0 walks every position of the wave's range, WIN = 1 the set bits of a row mask's image exactly as
//                       masked_stream_kernel does (kernels_mask.hip).  Also the centroid probe of a DOT call (the centroid matrix as
//                       one list, or a table's per-file segments): merge_kernel<S, true> / merge_probe_seg_kernel use keys for
//                       their order only.
//   dot_merge_kernel    the fold of the per-wave lists, one wave per query: rows, dist (ord undone), n_found; tie flags zeroed
//   dot_finish_kernel   range search: the range_* sort kernels run as order-only machinery (sqrt_out 0) and write the keys' high
//                       halves; this turns them back into dist in place
#include "stream_walk.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// dot_stream_kernel
//
// grid = (blocks_per_list, nprobe | nj | 1, nq); block = 256 threads = 4 independent waves, each owning a contiguous run of
// positions of one inverted list (probe == nullptr, WIN = 0 only: of the single list [single_begin, single_end)).
// WIN = 0: the run is walked in 64-row tiles.  WIN = 1: in 64-position windows of the mask's image (two words, funnel-shifted),
// clipped at the candidate cap; the set positions are compacted through the first 128 words of the wave's idle tile area into a
// queue whose first 64 entries live in one register, and a tile runs whenever 64 are queued and once more at the end -- a row the
// mask excludes is never loaded, positions stay the unmasked ones, and the waves add what they evaluated to embeddings_fetched
// (the (0, 0) block of a query adds n_cand[q] to candidate_rows), as masked_stream_kernel does.
// Outputs: stream_kernel's per-wave partial lists (STREAM_TOPK) / hit segments (STREAM_RANGE: hit iff dist <= radius).
// ------------------------------------------------------------------------------------
template <int CG, int S, int MODE, bool ALIGNED, int WIN>
__global__ __launch_bounds__(256) void dot_stream_kernel(const StreamArgs a, const MaskedArgs ma) {
    static_assert(MODE == STREAM_TOPK || MODE == STREAM_RANGE, "top-k lists or range hits");
    static_assert(tile_words<CG, false>() >= WindowQueue<false>::SCRATCH, "the compaction needs 128 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, false>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, false>();

    const uint32_t q = blockIdx.z, j = blockIdx.y + (MODE == STREAM_RANGE ? a.j0 : 0u);
    const WalkRange w = walk_range<WIN != 0>(a, q, j, wave);
    const float *qv = a.queries + (uint64_t)q * a.dim;

    WaveTopk<S> tk;
    if constexpr (MODE == STREAM_TOPK) tk.init();

    // what a tile's rows become: lane `lane` holds row my_srow at candidate position pos
    auto emit = [&](float sum, bool valid, uint64_t pos, uint32_t my_srow) {
        const float dist = 0.0f - sum;
        const uint64_t key = dot_key(sum, pos);
        if constexpr (MODE == STREAM_TOPK) tk.offer(valid ? key : KEY_EMPTY, my_srow, a.k, lane);
        else emit_range_hit(a, q, valid && dist <= a.radius, key, my_srow, lane);     // (a NaN distance never compares true)
    };

    if constexpr (WIN == 0) {
        for (uint64_t t0 = w.r0; t0 < w.r1; t0 += 64) {
            const uint32_t nvalid = (w.r1 - t0 < 64) ? (uint32_t)(w.r1 - t0) : 64u;
            const uint32_t lrow = (uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1;
            const uint32_t my_srow = storage_row(a, w.lbeg + t0 + lrow);
            const float sum = dot_tile<CG, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
            const uint64_t pos = w.cbase + t0 + (uint64_t)lane;
            emit(sum, (uint32_t)lane < nvalid && pos < w.lim, pos, my_srow);
        }
    } else {
        unsigned long long *st = stats_slot(ma.stats, q);
        stats_add_candidates(st, ma.n_cand, q, j);
        const uint32_t n_eval = filtered_walk<false>(
            w.lbeg, w.r0, w.r1, lds, lane, [&](uint64_t p, uint64_t, uint64_t, uint32_t &) { return image_window(ma.bits, p); },
            [&](const QueueTile &t) {
                const uint32_t my_srow = storage_row(a, w.lbeg + t.my_r);
                const float sum = dot_tile<CG, ALIGNED>(a, lds, qv, my_srow, t.nvalid, lane);
                emit(sum, (uint32_t)lane < t.nvalid, w.cbase + t.my_r, my_srow);           // (pos < lim by the clamp of the walk)
            });
        if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
    }

    if constexpr (MODE == STREAM_TOPK) write_partial_lists<S>(a.part_keys, a.part_vals, partial_base(a, q, j, wave, a.k), a.k, lane, tk.key, tk.val);
}

// (no SEQ chain: PQV_DOT has the 4-grouped form only)
template <int S, int MODE, int WIN>
static hipError_t launch_dot_s(const StreamArgs &a, const MaskedArgs &ma, hipStream_t s) {
    return dispatch_chunk<false>(a.dim, a.metric, [&](auto cg, auto, auto aligned) {
        dim3 grid(a.blocks_per_list, !a.probe ? 1u : MODE == STREAM_RANGE ? a.nj : a.nprobe, a.nq);
        hipLaunchKernelGGL((dot_stream_kernel<cg.value, S, MODE, aligned.value, WIN>), grid, dim3(256), 0, s, a, ma);
        return hipGetLastError();
    });
}

template <int WIN>
static hipError_t launch_dot_w(const StreamArgs &a, const MaskedArgs &ma, StreamMode mode, hipStream_t s) {
    if (a.nq == 0 || a.blocks_per_list == 0) return hipSuccess;
    if (mode == STREAM_RANGE) {
        if (a.nj == 0) return hipSuccess;
        if (!a.probe) return hipErrorInvalidValue;
        return launch_dot_s<1, STREAM_RANGE, WIN>(a, ma, s);
    }
    if (mode != STREAM_TOPK) return hipErrorInvalidValue;
    if (a.probe && a.nprobe == 0) return hipSuccess;
    return dispatch_list_slots(a.k, [&](auto S) { return launch_dot_s<S.value, STREAM_TOPK, WIN>(a, ma, s); });
}

hipError_t launch_dot_stream(const StreamArgs &a, const MaskedArgs *ma, StreamMode mode, hipStream_t s) {
    if (a.zero_u32 || (a.rows_per_block % 256) != 0 || a.rows_per_block == 0) return hipErrorInvalidValue;
    if (a.probe && (!a.list_off || !a.cand_base)) return hipErrorInvalidValue;
    if (!ma) return launch_dot_w<0>(a, MaskedArgs{}, mode, s);
    if (!ma->bits || !a.probe) return hipErrorInvalidValue;
    return launch_dot_w<1>(a, *ma, mode, s);
}

// ------------------------------------------------------------------------------------
// dot_merge_kernel: one wave per query folds the per-wave lists [n_part][k_part] into the k smallest keys and writes the first
// k_out: reported rows, dist = the key's high half with ord undone, 0xFFFFFFFF / +inf past n_found; tie_flag[q] = 0 (there is
// no reference heap whose history a tie could depend on).
// ------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void dot_merge_kernel(const MergeArgs a) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    WaveTopk<S> tk;
    tk.init();
    const uint64_t total = (uint64_t)a.n_part * a.k_part;
    const uint64_t *pk = a.part_keys + (uint64_t)q * total;
    const uint32_t *pv = a.part_vals + (uint64_t)q * total;
    // pre-filter (k <= 64): the k-th smallest of the 64 lane minima bounds the k-th smallest overall, so only keys at or below it
    // reach the serial insertion (merge_kernel's cut)
    uint64_t cut = KEY_EMPTY;
    if (S == 1 && total > 128) {
        uint64_t lmin = KEY_EMPTY;
        for (uint64_t i = lane; i < total; i += 64) { const uint64_t key = pk[i]; lmin = key < lmin ? key : lmin; }
        uint32_t dummy = 0;
        bitonic_sort64(lmin, dummy, lane);
        cut = readlane_u64(lmin, (int)a.k - 1);
    }
    for (uint64_t i = 0; i < total; i += 64) {
        const uint64_t idx = i + lane;
        uint64_t key = KEY_EMPTY;
        uint32_t val = 0xFFFFFFFFu;
        if (idx < total) { key = pk[idx]; val = pv[idx]; }
        if (key > cut) key = KEY_EMPTY;
        if (__ballot(key != KEY_EMPTY) != 0ull) tk.offer(key, val, a.k, lane);
    }
    const uint32_t k_out = a.k_out ? a.k_out : a.k;
    uint32_t found = 0;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        const bool have = e < a.k && tk.key[s] != KEY_EMPTY;
        found += (uint32_t)__popcll(__ballot(have && e < k_out));
        if (e < k_out) {
            uint32_t row = 0xFFFFFFFFu;
            float d = INFINITY;
            if (have) {
                row = a.ids ? a.ids[tk.val[s]] : tk.val[s];
                d = dot_unord((uint32_t)(tk.key[s] >> 32));
            }
            a.row_idx[(uint64_t)q * k_out + e] = row;
            a.dist[(uint64_t)q * k_out + e] = d;
        }
    }
    if (a.n_found && lane == 0) a.n_found[q] = found;
    if (a.tie_flag && lane == 0) a.tie_flag[q] = 0u;
}

hipError_t launch_dot_merge(const MergeArgs &a, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (a.cand_keys || a.cand_lb || a.part_flags || a.k == 0 || (a.k_out ? a.k_out : a.k) > a.k) return hipErrorInvalidValue;
    return dispatch_list_slots(a.k, [&](auto S) {
        hipLaunchKernelGGL(dot_merge_kernel<S.value>, dim3(a.nq), dim3(64), 0, s, a);
        return hipGetLastError();
    });
}

// dist[i] = the distance whose ord bits dist[i] holds (range search write-out), i < n
__global__ __launch_bounds__(256) void dot_finish_kernel(float *dist, uint64_t n) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
        dist[i] = dot_unord(reinterpret_cast<const uint32_t *>(dist)[i]);
}

hipError_t launch_dot_finish(float *dist, uint64_t n, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(dot_finish_kernel, dim3((uint32_t)(blocks < 4096 ? blocks : 4096)), dim3(256), 0, s, dist, n);
    return hipGetLastError();
}

}  // namespace pqv
