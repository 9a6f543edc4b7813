// kernels_mask.hip -- gfx950 kernels of the row-masked searches (pqv.h: pqv_row_mask): mask_layout_kernel (allow bytes in row
// order -> a bitset indexed by LIST POSITION) and masked_stream_kernel (stream_kernel's exact distance pass over the allowed
// positions only) -- and of the per-query key filters (pqv.h: pqv_row_keys): key_layout_kernel (a key column in row order -> list
// position order) and masked_stream_kernel's keyed instantiations, whose windows come from comparing keys.  The screened paths take their thresholds from sampled rows; a threshold from a row the mask excludes is no
// bound on the masked answer, so masked calls always run this exact pass.
#include "stream_walk.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// mask_layout_kernel: bit p of `bits` = allowed[ids[p]] for list position p (ids: list position -> the row a call reports, a
// searcher's d_ids in every layout).  One thread per position; a wave's 64 answers are one __ballot word, stored by lane 0
// (positions start at a multiple of 64 per wave, so the word index is p / 64); positions >= n_pos give zero bits.  The allowed
// total: a popcount and one atomicAdd per wave.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_layout_kernel(const uint8_t *allowed, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos,
                                                          uint64_t *bits, uint64_t n_words, unsigned long long *count) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (p < n_pos) {
        const uint64_t r = ids ? ids[p] : p;
        on = r < n_rows && allowed[r] != 0;
    }
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63) == 0) {
        const uint64_t w = p >> 6;
        if (w < n_words) bits[w] = m;
        if (m) atomicAdd(count, (unsigned long long)__popcll(m));
    }
}

hipError_t launch_mask_layout(const uint8_t *allowed, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos, uint64_t *bits,
                              uint64_t n_words, unsigned long long *count, hipStream_t s) {
    // every word of the image is written: one wave per word, n_words >= ceil(n_pos / 64) + 1 (masked_stream_kernel reads two words)
    const uint64_t blocks = (n_words * 64 + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_layout_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, allowed, n_rows, ids, n_pos, bits, n_words, count);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// key_layout_kernel: key_pos[p] = values[ids[p]] for list position p (T: the column's width as an unsigned word -- the values are
// copied, never interpreted), zero for positions >= n_pos; one thread per entry of the padded image, so the stores of a wave are
// one coalesced 256- / 512-byte line.  With validity bytes: bit p of valid_pos = valid[ids[p]] != 0, a wave's __ballot word
// stored by lane 0, exactly as mask_layout_kernel writes a mask's image.
// ------------------------------------------------------------------------------------
template <class T>
__global__ __launch_bounds__(256) void key_layout_kernel(const T *values, const uint8_t *valid, uint64_t n_rows, const uint32_t *ids,
                                                         uint64_t n_pos, T *key_pos, uint64_t *valid_pos, uint64_t n_words) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    T v = 0;
    bool on = false;
    if (p < n_pos) {
        const uint64_t r = ids ? ids[p] : p;
        if (r < n_rows) {
            v = values[r];
            on = !valid || valid[r] != 0;
        }
    }
    if (p < n_words * 64) key_pos[p] = v;
    if (valid_pos) {
        const uint64_t m = __ballot(on);
        const uint64_t w = p >> 6;
        if ((threadIdx.x & 63) == 0 && w < n_words) valid_pos[w] = m;
    }
}

hipError_t launch_key_layout(const void *values, const uint8_t *valid, uint32_t elem_size, uint64_t n_rows, const uint32_t *ids,
                             uint64_t n_pos, void *key_pos, uint64_t *valid_pos, uint64_t n_words, hipStream_t s) {
    if (elem_size != 4 && elem_size != 8) return hipErrorInvalidValue;
    const uint64_t blocks = (n_words * 64 + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    uint64_t *vp = valid ? valid_pos : nullptr;
    if (elem_size == 4)
        hipLaunchKernelGGL(key_layout_kernel<uint32_t>, dim3((uint32_t)blocks), dim3(256), 0, s, static_cast<const uint32_t *>(values),
                           valid, n_rows, ids, n_pos, static_cast<uint32_t *>(key_pos), vp, n_words);
    else
        hipLaunchKernelGGL(key_layout_kernel<uint64_t>, dim3((uint32_t)blocks), dim3(256), 0, s, static_cast<const uint64_t *>(values),
                           valid, n_rows, ids, n_pos, static_cast<uint64_t *>(key_pos), vp, n_words);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// masked_stream_kernel
//
// stream_kernel's grid (row block, probe rank, query), its 4 independent waves per block and its chain tile (l2_tile: REF4 groups
// / SEQ squares, dim % 4 tails, unaligned rows).  The walk, the queue, the key test and the outputs are stream_walk.hpp's pieces,
// which every other filtered form composes too; what follows describes them as this kernel uses them.
// What differs is WHICH rows fill a 64-row tile: a wave walks its position range [r0, r1) of the list in 64-position windows,
// reads the window's mask word (lbeg + r0 is not 64-aligned: two words, funnel-shifted), drops the bits at or beyond the
// candidate cap (max_pos / pair_end) and compacts the set positions into a queue, rank from mbcnt.  A chain tile runs whenever 64
// positions are queued, and once more at the end of the range -- so the f32 bytes read are (considered rows) x 4 dim and a row
// the mask excludes is never loaded.  Keys stay (d2 bits << 32) | (u32)(cbase + position in list): the unmasked positions.
//
// The queue: its first 64 entries live in a register (lane i holds entry i), at most 63 of them between two windows.  A window's
// compaction goes through the first 128 words of the wave's tile area in LDS, which is idle between two chain tiles -- no LDS
// beside the tile, so an instantiation's occupancy is its stream_kernel twin's (CG = 32: 32 KiB per block; a queue of its own
// would take the fifth block per CU away).
//
// WIN, the source of a window's 64 bits: 0 the mask's image as above; 1 / 2 a key column (i32 / i64) in list-position order -- lane
// l loads key_pos[lbeg + w0 + l] (one coalesced 256- / 512-byte read per window), compares it as an i64 against the query's key
// (wave-uniform, loaded once) and the __ballot of the comparison is the window, ANDed with the funnel-shifted words of valid_pos
// and of a shared mask where the call has them, and clipped like a mask's.  Everything behind the window is shared.
//
// WIN 3 / 4 (i32 / i64), a per-query RANGE (pqv.h: PQV_KEY_RANGE): the same load, the bounds lo / hi wave-uniform and loaded once,
// the window the __ballot of lo <= kv && kv <= hi.  WIN 5 / 6, a per-query set (PQV_KEY_IN): the block copies its query's slice
// vals[lims[q] .. lims[q + 1]) -- never more than KEY_SET_MAX values, never anything outside the slice -- into 8 KiB of LDS behind
// the tile area before the first window (the kernel's one __syncthreads: every wave reaches it, the waves are independent behind
// it) and a lane's key is looked up by a halving search whose trip count depends on the slice length only; the window is the
// __ballot of "found".  An empty slice walks nothing.  A slice that is not ascending finds some keys and misses others; every
// index the search forms stays below the slice length.
//
// rank_limit (STREAM_TOPK, optional; pqv_topk_expand): the blocks of probe ranks j >= rank_limit[q] store empty lists and end.
// j == 0 is below every limit (>= 1), so the candidate_rows word is still added once per query.
//
// Outputs: stream_kernel's (per-wave partial lists / hit segments).  Each wave adds the rows it evaluated to the
// embeddings_fetched word of the query's statistics slot; the (0, 0) block of a query adds n_cand[q] to candidate_rows.
// ------------------------------------------------------------------------------------
template <int WIN> struct WinArgs { using type = KeyFilterArgs; };
template <> struct WinArgs<0> { using type = MaskedArgs; };
template <> struct WinArgs<1> { using type = KeyedArgs; };
template <> struct WinArgs<2> { using type = KeyedArgs; };
template <> struct WinArgs<7> { using type = MaskedArgs; };      // WIN 7: no filter at all -- every window is all ones (launch_limited_stream)

template <int CG, int S, int MODE, bool SEQ, bool ALIGNED, int WIN = 0>
__global__ __launch_bounds__(256) void masked_stream_kernel(const StreamArgs a, const typename WinArgs<WIN>::type ma) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<false>::SCRATCH, "the compaction needs 128 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y + (MODE == STREAM_RANGE ? a.j0 : 0u);
    if constexpr (MODE == STREAM_TOPK) {
        // a rank at or beyond the query's limit (pqv_topk_expand) walks nothing: that one word is all the block loads, its four
        // waves' lists go out EMPTY for the final merge (block-uniform: nobody is left waiting at the IN forms' barrier)
        if (ma.rank_limit && j >= ma.rank_limit[q]) {
            const uint64_t base = partial_base(a, q, j, wave, a.k);
            for (uint32_t e = lane; e < a.k; e += 64) {
                a.part_keys[base + e] = KEY_EMPTY;
                a.part_vals[base + e] = 0xFFFFFFFFu;
            }
            return;
        }
    }
    WalkRange w = walk_range<true>(a, q, j, wave);
    unsigned long long *st = stats_slot(ma.stats, q);
    stats_add_candidates(st, ma.n_cand, q, j);

    KeyTest<(WIN == 0 || WIN == 7) ? 0 : (WIN - 1) / 2> kt;       // WIN 1 / 2: EQ, 3 / 4: RANGE, 5 / 6: IN
    if constexpr (WIN == 1 || WIN == 2) kt.lo = ma.qkeys[q];
    if constexpr (WIN == 3 || WIN == 4) {
        kt.lo = static_cast<const int64_t *>(ma.a)[q];
        kt.hi = static_cast<const int64_t *>(ma.b)[q];
    }
    if constexpr (WIN == 5 || WIN == 6) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        kt.setup_in(ma.a, ma.b, q, set_lds);
        if (kt.empty()) w.r1 = w.r0;      // (nothing matches: no window is read)
    }

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveTopk<S> tk;
    if constexpr (MODE == STREAM_TOPK) tk.init();

    const uint32_t n_eval = filtered_walk<false>(
        w.lbeg, w.r0, w.r1, lds, lane,
        [&](uint64_t p, uint64_t, uint64_t, uint32_t &) {
            if constexpr (WIN == 0) {
                return image_window(ma.bits, p);
            } else if constexpr (WIN == 7) {
                return ~0ull;
            } else {
                uint64_t win = kt.window(ma.key_pos, (WIN & 1) != 0, ma.valid_pos, p, lane);
                if (ma.bits) win &= image_window(ma.bits, p);
                return win;
            }
        },
        [&](const QueueTile &t) {
            const uint32_t my_srow = storage_row(a, w.lbeg + t.my_r);
            const float sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, t.nvalid, lane);
            const uint64_t pos = w.cbase + t.my_r;
            const bool valid = (uint32_t)lane < t.nvalid;           // (pos < lim by the clamp of the walk)
            if constexpr (MODE == STREAM_TOPK) tk.offer(valid ? l2_key(sum, pos) : KEY_EMPTY, my_srow, a.k, lane);
            else emit_l2_range_hit(a, q, valid, sum, pos, my_srow, lane);
        });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    if constexpr (MODE == STREAM_TOPK) write_partial_lists<S>(a.part_keys, a.part_vals, partial_base(a, q, j, wave, a.k), a.k, lane, tk.key, tk.val);
}

template <int S, int MODE, int WIN>
static hipError_t launch_masked_s(const StreamArgs &a, const typename WinArgs<WIN>::type &ma, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, MODE == STREAM_RANGE ? a.nj : a.nprobe, a.nq);
        hipLaunchKernelGGL((masked_stream_kernel<cg.value, S, MODE, seq.value, aligned.value, WIN>), grid, dim3(256), 0, s, a, ma);
        return hipGetLastError();
    });
}

template <int WIN>
static hipError_t launch_masked_w(const StreamArgs &a, const typename WinArgs<WIN>::type &ma, StreamMode mode, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0) return hipSuccess;
    if (mode == STREAM_RANGE) return a.nj == 0 ? hipSuccess : launch_masked_s<1, STREAM_RANGE, WIN>(a, ma, s);
    if (mode != STREAM_TOPK) return hipErrorInvalidValue;
    if (a.nprobe == 0) return hipSuccess;
    return dispatch_list_slots(a.k, [&](auto S) { return launch_masked_s<S.value, STREAM_TOPK, WIN>(a, ma, s); });
}

hipError_t launch_masked_stream(const StreamArgs &a, const MaskedArgs &ma, StreamMode mode, hipStream_t s) {
    if (!ma.bits) return hipErrorInvalidValue;
    return launch_masked_w<0>(a, ma, mode, s);
}

// The plain walk under per-query rank limits (pqv_topk_depth on the exact stream): no mask, every position of a walked list is a
// candidate and its key is stream_kernel's; the blocks of a rank at or beyond rank_limit[q] store empty lists and end.
hipError_t launch_limited_stream(const StreamArgs &a, const MaskedArgs &ma, hipStream_t s) {
    if (ma.bits || !ma.rank_limit) return hipErrorInvalidValue;
    return launch_masked_w<7>(a, ma, STREAM_TOPK, s);
}

hipError_t launch_keyed_stream(const StreamArgs &a, const KeyedArgs &ka, StreamMode mode, hipStream_t s) {
    if (!ka.key_pos || !ka.qkeys) return hipErrorInvalidValue;
    if (ka.elem_size == 4) return launch_masked_w<1>(a, ka, mode, s);
    if (ka.elem_size == 8) return launch_masked_w<2>(a, ka, mode, s);
    return hipErrorInvalidValue;
}

hipError_t launch_key_filter_stream(const StreamArgs &a, const KeyFilterArgs &fa, StreamMode mode, hipStream_t s) {
    if (fa.kind == 0) {       // PQV_KEY_EQ: the keyed call, unchanged
        KeyedArgs ka = fa;
        ka.qkeys = static_cast<const int64_t *>(fa.a);
        return launch_keyed_stream(a, ka, mode, s);
    }
    if (!fa.key_pos || !fa.a || !fa.b || (fa.elem_size != 4 && fa.elem_size != 8)) return hipErrorInvalidValue;
    if (fa.kind == 1) return fa.elem_size == 4 ? launch_masked_w<3>(a, fa, mode, s) : launch_masked_w<4>(a, fa, mode, s);
    if (fa.kind == 2) return fa.elem_size == 4 ? launch_masked_w<5>(a, fa, mode, s) : launch_masked_w<6>(a, fa, mode, s);
    return hipErrorInvalidValue;
}

__global__ void touch_mask_kernel() {}
hipError_t touch_mask(hipStream_t s) {
    hipLaunchKernelGGL(touch_mask_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace pqv
