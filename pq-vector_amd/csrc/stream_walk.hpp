// stream_walk.hpp -- the pieces every streaming distance pass is composed of, each ONCE.  stream_kernel (kernels_probe.hip),
// masked_stream_kernel (kernels_mask.hip), dot_stream_kernel (kernels_dot.hip), distinct_stream_kernel, grouped_stream_kernel and
// their filtered forms (kernels_distinct.hip, kernels_grouped.hip, kernels_distinct_filter.hip), filter_count_kernel
// (kernels_expand.hip) and group_expand_kernel (kernels_group_expand.hip) differ only in where a window's bits come from and what a tile's rows are offered to; everything else is here:
//
//   chain_tile / l2_tile / dot_tile   the distance chain of one 64-row tile, in the reference's order of operations
//   WalkRange / walk_range            the prologue: probed list, candidate base, cap, the wave's position range
//   WindowQueue / filtered_walk       the walk over 64-position windows: compaction into a queue, a tile per 64 queued rows
//   PartitionSeq / walk_seq_windows   a key partition's candidate sequence: position -> list position, a wave's windows; the filtered
//                                     walk of any such sequence (a caller's candidate list: RowsSeq, kernels_rows.hip)
//   KeyTest                           a query's key test (EQ / RANGE / IN): setup once per block, one window per call
//   GroupSet                          the k groups of a grouped call's pass 2: staged in LDS, membership and slot per key
//   distinct_tile / grouped_tile ...  what a distinct / grouped kernel shares with its filtered twin: images, tile, list write-out
//   stats_slot, l2_key, emit_range_hit, write_partial_lists     the statistics slot, a candidate's key, the two output formats
//   dispatch_chunk (host)             the chunk choice (CG, SEQ, ALIGNED) of every launcher
//   dispatch_list_slots (host)        the list length choice (S) of every launcher
//
// The forms promise results bit-identical to each other and the tests compare form against form: a change to the chain, the
// clamps or the barrier placement belongs here, where every form gets it.
#ifndef PQV_STREAM_WALK_HPP
#define PQV_STREAM_WALK_HPP
#include "device_common.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// The chain tile.  A wave's tile area is [chain element e][row r], XOR-swizzled (column r ^ (e & 63)) so that both the
// group-major writes and the row-major chain reads are bank-conflict-free without padding: CG = 64 uses exactly 64 KiB per block.
// ------------------------------------------------------------------------------------
template <int CG, bool SEQ>
constexpr int tile_words() { return CG * (SEQ ? 4 : 1) * 64; }

__device__ __forceinline__ float &lds_at(float *lds, uint32_t e, uint32_t r) { return lds[e * 64 + (r ^ (e & 63))]; }

// storage row of list position lpos
__device__ __forceinline__ uint32_t storage_row(const StreamArgs &a, uint64_t lpos) { return a.row_of ? a.row_of[lpos] : (uint32_t)lpos; }

// Lane r returns row r's chain for r < nvalid (my_srow: the storage row of tile row `lane`, clamped by the caller so that every
// address is in range).  For a chunk of CG float4 groups of the dimension:
//   1. every load instruction reads 64 x 16 B, fully coalesced (CG = 64: one 1 KiB row segment; CG = 32: two 512 B segments), NB
//      instructions in flight;
//   2. each lane turns its float4 into the reference's per-group partial t = ((d0^2 + d1^2) + d2^2) + d3^2 (PQV_L2SQ_REF4), four
//      squares (SEQ: PQV_L2SQ_SEQ) or t = ((q0 x0 + q1 x1) + q2 x2) + q3 x3 (DOT) and parks it in the tile;
//   3. lane r then replays row r's serial chain sum += t_g in ascending g -- the one part of the reference arithmetic that cannot
//      be re-associated -- and the dim % 4 tail element by element (index.rs:461-480).
// Every operation is a rounded f32 one: the units are built with -ffp-contract=off.
template <int CG, bool SEQ, bool ALIGNED, bool DOT>
__device__ __forceinline__ float chain_tile(const StreamArgs &a, float *lds, const float *qv, uint32_t my_srow, uint32_t nvalid, int lane) {
    constexpr int RPI = 64 / CG;        // rows per load instruction
    constexpr int NI = CG;              // load instructions per 64-row tile
    constexpr int EPL = SEQ ? 4 : 1;    // LDS values per lane item
    constexpr int NB = 8;               // loads in flight per lane
    static_assert(NI % NB == 0, "NI must be a multiple of NB");
    static_assert(!(DOT && SEQ), "the products chain has the 4-grouped form only");
    const uint32_t dim = a.dim;
    const uint32_t G = dim >> 2;
    const uint32_t tail = dim & 3u;
    const int g_in = lane % CG;      // my float4 group inside a chunk
    const int row_in = lane / CG;    // my row inside a load instruction

    float sum = 0.0f;
    for (uint32_t c0 = 0; c0 < G; c0 += CG) {
        const uint32_t ng = (G - c0 < (uint32_t)CG) ? (G - c0) : (uint32_t)CG;
        const bool gvalid = (uint32_t)g_in < ng;
        const uint32_t goff = (c0 + (gvalid ? g_in : 0)) * 4;
        const float4 qq = load4<ALIGNED>(qv + goff);

#pragma unroll 1
        for (int ib = 0; ib < NI; ib += NB) {
            float4 x[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                uint32_t rr = (uint32_t)((ib + u) * RPI + row_in);
                if (rr >= nvalid) rr = nvalid - 1;
                const uint32_t srow = (uint32_t)__shfl((int)my_srow, (int)rr, 64);
                x[u] = load4<ALIGNED>(a.mat + (uint64_t)srow * dim + goff);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int rr = (ib + u) * RPI + row_in;
                if constexpr (DOT) {
                    float t = qq.x * x[u].x + qq.y * x[u].y;
                    t = t + qq.z * x[u].z;
                    t = t + qq.w * x[u].w;
                    if (gvalid) lds_at(lds, g_in, rr) = t;
                } else {
                    const float d0 = qq.x - x[u].x, d1 = qq.y - x[u].y;
                    const float d2 = qq.z - x[u].z, d3 = qq.w - x[u].w;
                    if constexpr (SEQ) {
                        if (gvalid) {
                            lds_at(lds, g_in * 4 + 0, rr) = d0 * d0;
                            lds_at(lds, g_in * 4 + 1, rr) = d1 * d1;
                            lds_at(lds, g_in * 4 + 2, rr) = d2 * d2;
                            lds_at(lds, g_in * 4 + 3, rr) = d3 * d3;
                        }
                    } else {
                        float t = d0 * d0 + d1 * d1;
                        t = t + d2 * d2;
                        t = t + d3 * d3;
                        if (gvalid) lds_at(lds, g_in, rr) = t;
                    }
                }
            }
        }
        wave_lds_fence();
        const uint32_t nchain = ng * EPL;
        uint32_t e = 0;
        for (; e + 8 <= nchain; e += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = lds_at(lds, e + u, lane);
#pragma unroll
            for (int u = 0; u < 8; ++u) sum = sum + v[u];
        }
        for (; e < nchain; ++e) sum = sum + lds_at(lds, e, lane);
        wave_lds_fence();
    }
    if (tail) {  // scalar tail of squared_l2_distance (index.rs:474-478)
        const float *xr = a.mat + (uint64_t)my_srow * dim + (uint64_t)G * 4;
        const float *qt = qv + (uint64_t)G * 4;
        for (uint32_t e = 0; e < tail; ++e) {
            if constexpr (DOT) {
                sum = sum + qt[e] * xr[e];
            } else {
                const float d = qt[e] - xr[e];
                sum = sum + d * d;
            }
        }
    }
    return sum;
}

template <int CG, bool SEQ, bool ALIGNED>
__device__ __forceinline__ float l2_tile(const StreamArgs &a, float *lds, const float *qv, uint32_t my_srow, uint32_t nvalid, int lane) {
    return chain_tile<CG, SEQ, ALIGNED, false>(a, lds, qv, my_srow, nvalid, lane);
}
template <int CG, bool ALIGNED>
__device__ __forceinline__ float dot_tile(const StreamArgs &a, float *lds, const float *qv, uint32_t my_srow, uint32_t nvalid, int lane) {
    return chain_tile<CG, false, ALIGNED, true>(a, lds, qv, my_srow, nvalid, lane);
}

// a candidate's key: ascending keys = ascending (d2, candidate position)
__device__ __forceinline__ uint64_t l2_key(float d2, uint64_t pos) { return ((uint64_t)__float_as_uint(d2) << 32) | (uint64_t)(uint32_t)pos; }
// PQV_DOT (kernels_dot.hip): distances are signed, so a key carries ord(dist), the order-preserving map of f32 bits to u32
// (negative: all bits flipped; else: the sign bit set); dot_key: the key of the products chain `sum`, dist = 0.0f - sum
__device__ __forceinline__ uint32_t dot_ord(float d) {
    const uint32_t b = __float_as_uint(d);
    return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u);
}
__device__ __forceinline__ float dot_unord(uint32_t o) {
    return __uint_as_float((o >> 31) ? o ^ 0x80000000u : ~o);
}
__device__ __forceinline__ uint64_t dot_key(float sum, uint64_t pos) { return ((uint64_t)dot_ord(0.0f - sum) << 32) | (uint64_t)(uint32_t)pos; }

// ------------------------------------------------------------------------------------
// The walk range: block (row block x, probe rank j, query q), wave `wave` of 4.  The list of rank j (probe == nullptr, unclamped
// forms only: the single list [single_begin, single_end)), its first candidate position cbase, the cap lim (pair_end / max_pos)
// and the wave's positions [r0, r1) of the list.  CLAMP: positions at or beyond the cap are no candidates and the walk ends
// there, BEFORE any filter -- their bits are never looked at.  Without it the caller tests pos < lim per row.
// ------------------------------------------------------------------------------------
template <class T>
__device__ __forceinline__ T uniform_word(const T *p) {
    return *(const __attribute__((address_space(4))) T *)(uintptr_t)p;
}

struct WalkRange {
    uint64_t lbeg, cbase, lim, r0, r1;
};

template <bool CLAMP>
__device__ __forceinline__ WalkRange walk_range(const StreamArgs &a, uint32_t q, uint32_t j, int wave) {
    WalkRange w;
    uint64_t lend;
    w.lim = a.max_pos;
    if (CLAMP || a.probe) {
        // (block-uniform words of arrays no kernel of the pass writes: read as load4_uniform reads its operands, so that they
        // stay scalar loads whatever stores and atomics the kernel around them holds)
        const uint64_t at = (uint64_t)q * a.nprobe + j;
        const uint32_t c = uniform_word(a.probe + at);
        w.lbeg = uniform_word(a.list_off + c);
        lend = uniform_word(a.list_off + c + 1);
        w.cbase = uniform_word(a.cand_base + at);
        if (a.pair_end) w.lim = uniform_word(a.pair_end + at);
    } else {
        w.lbeg = a.single_begin;
        lend = a.single_end;
        w.cbase = 0;
    }
    uint64_t len = lend - w.lbeg;
    if constexpr (CLAMP) {
        const uint64_t room = w.lim > w.cbase ? w.lim - w.cbase : 0;
        if (len > room) len = room;
    }
    const uint64_t wrows = a.rows_per_block / 4;
    w.r0 = (uint64_t)blockIdx.x * a.rows_per_block + (uint64_t)wave * wrows;
    w.r1 = w.r0 + wrows;
    if (w.r1 > len) w.r1 = len;
    return w;
}

// the statistics slot of query q (nullptr: no statistics)
__device__ __forceinline__ unsigned long long *stats_slot(unsigned long long *stats, uint32_t q) {
#ifdef PQV_PROFILE_PHASES
    return stats;
#else
    return stats ? stats + 8 + 16 * (q % STATS_SLOTS) : nullptr;
#endif
}
// the (0, 0) block of a query adds the probe merge's uncapped total to candidate_rows
__device__ __forceinline__ void stats_add_candidates(unsigned long long *st, const uint64_t *n_cand, uint32_t q, uint32_t j) {
    if (n_cand && st && blockIdx.x == 0 && j == 0 && threadIdx.x == 0) atomicAdd(&st[2], (unsigned long long)n_cand[q]);
}

// ------------------------------------------------------------------------------------
// The window queue.  A window's set positions are compacted (rank from mbcnt) behind what is already queued; the first 64
// entries live in a register (lane i holds entry i), at most 63 of them between two windows.  The compaction goes through the
// first SCRATCH words of the wave's tile area, which is idle between two chain tiles -- no LDS beside the tile.  PAYLOAD: every
// entry carries one more word (grouped: the slot) through the second half of the scratch.
// ------------------------------------------------------------------------------------
struct QueueTile {
    uint32_t nvalid;    // rows of the chain tile to run (0: none)
    uint32_t my_r;      // list offset of tile row `lane` (clamped: every address in range)
    uint32_t my_x;      // ... and its payload
};

template <bool PAYLOAD>
struct WindowQueue {
    static constexpr int SCRATCH = PAYLOAD ? 256 : 128;
    uint32_t *cq;           // compaction scratch: 128 list offsets (then 128 payload words)
    uint32_t pend = 0;      // queue entry `lane` (a list offset, < 2^32 as every candidate position), meaningful for lane < qn
    uint32_t pend_x = 0;    // ... and its payload
    uint32_t qn = 0;        // queued entries, < 64 between two windows (wave-uniform)

    // queue the set positions w0 + l of `win` (x: lane l's payload); a full tile comes back once 64 are queued
    __device__ __forceinline__ QueueTile push(uint64_t win, uint64_t w0, uint32_t x, int lane) {
        QueueTile t{0u, 0u, 0u};
        uint32_t *cs = cq + 128;
        const uint32_t cnt = (uint32_t)__popcll(win);
        if (cnt == 0) return t;
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(win >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)win, 0u));
        if ((uint32_t)lane < qn) {
            cq[lane] = pend;
            if constexpr (PAYLOAD) cs[lane] = pend_x;
        }
        if ((win >> lane) & 1ull) {
            cq[qn + rank] = (uint32_t)(w0 + (uint64_t)lane);
            if constexpr (PAYLOAD) cs[qn + rank] = x;
        }
        wave_lds_fence();
        const uint32_t total = qn + cnt;                   // <= 127
        const uint32_t first = cq[lane], over = cq[64 + lane];
        uint32_t first_x = 0, over_x = 0;
        if constexpr (PAYLOAD) { first_x = cs[lane]; over_x = cs[64 + lane]; }
        wave_lds_fence();
        if (total >= 64) {
            t.my_r = first; t.my_x = first_x; t.nvalid = 64u;
            pend = over; pend_x = over_x; qn = total - 64;
        } else {
            pend = first; pend_x = first_x; qn = total;
        }
        return t;
    }
    // past the range: what is left in the queue is the last tile
    __device__ __forceinline__ QueueTile flush(int lane) {
        QueueTile t{0u, 0u, 0u};
        if (qn) {
            const uint32_t last = (uint32_t)__shfl((int)pend, (int)(qn - 1), 64);
            t.my_r = (uint32_t)lane < qn ? pend : last;
            t.my_x = pend_x;
            t.nvalid = qn; qn = 0;
        }
        return t;
    }
};

// The filtered walk of one wave over positions [r0, r1) of a list.  window(p, w0, clip, x) returns the 64 bits of positions
// lbeg + w0 .. + 63 (p = lbeg + w0; clip: the positions below r1, which the walk ANDs in whatever comes back; x: lane l's payload,
// PAYLOAD forms); tile(t) runs a chain tile.  A tile runs whenever 64 positions are queued and once more at the end of the range,
// so a row the filter excludes is never loaded.  Returns the rows evaluated (wave-uniform).
template <bool PAYLOAD, class W, class T>
__device__ __forceinline__ uint32_t filtered_walk(uint64_t lbeg, uint64_t r0, uint64_t r1, float *lds, int lane, W &&window, T &&tile) {
    WindowQueue<PAYLOAD> wq;
    wq.cq = reinterpret_cast<uint32_t *>(lds);
    uint32_t n_eval = 0;
    for (uint64_t w0 = r0;; w0 += 64) {
        const bool last = w0 >= r1;
        QueueTile t;
        if (!last) {
            const uint64_t clip = r1 - w0 < 64 ? (1ull << (r1 - w0)) - 1ull : ~0ull;
            uint32_t x = 0;
            const uint64_t win = window(lbeg + w0, w0, clip, x) & clip;
            t = wq.push(win, w0, x, lane);
        } else {
            t = wq.flush(lane);
        }
        if (t.nvalid) {
            n_eval += t.nvalid;
            tile(t);
        }
        if (last) break;
    }
    return n_eval;
}

// ------------------------------------------------------------------------------------
// A key partition's candidate sequence (kernels_partition.hip, kernels_partition_group.hip; launch_partition_span's outputs): query
// q's sequence has `total` positions, known on the device only.  entry(seq) maps a position to its partition entry -- one span (EQ /
// RANGE): span_beg[q] + seq; IN: the first span whose inclusive prefix sum exceeds seq, found by a halving search over the query's
// n_span[q] <= KEY_SET_MAX sums (read through the caches: no LDS beside the tile) -- and loads the entry's list position.
// windows(wave, lane, f): wave w of block x takes the 64-position windows (turn * gridDim.x + x) * 4 + w for turn = 0, 1, ... while
// they begin below `limit`; f(w0, nvalid, seq, lpos) gets the window's first position, its positions inside the sequence, and lane
// l's sequence position and list position, both clamped to the window's last one.
// ------------------------------------------------------------------------------------
struct PartitionSeq {
    uint32_t total, n_span, beg0;
    bool in_set;
    const uint32_t *sbeg, *send, *pos;

    __device__ __forceinline__ void setup(const PartitionArgs &pa, uint32_t q) {
        total = (uint32_t)uniform_word(pa.n_cand + q);       // (saturated below 2^32 by the span kernel)
        in_set = pa.kind == 2;
        n_span = in_set ? uniform_word(pa.n_span + q) : 1u;
        sbeg = pa.span_beg + (in_set ? (uint64_t)q * KEY_SET_MAX : (uint64_t)q);
        send = in_set ? pa.span_end + (uint64_t)q * KEY_SET_MAX : nullptr;
        beg0 = total ? uniform_word(sbeg) : 0u;
        pos = pa.pos;
    }
    // the list position of sequence position seq < total
    __device__ __forceinline__ uint32_t entry(uint32_t seq) const {
        uint32_t at = beg0 + seq;
        if (in_set) {
            uint32_t i = 0;
            for (uint32_t span = n_span; span > 1;) {       // (wave-uniform trip count; i + half - 1 < n_span)
                const uint32_t half = span >> 1;
                if (send[i + half - 1] <= seq) i += half;
                span -= half;
            }
            at = sbeg[i] + (seq - (i ? send[i - 1] : 0u));
        }
        return pos[at];
    }
    template <class F>
    __device__ __forceinline__ void windows(uint32_t limit, int wave, int lane, F &&f) const {
        const uint64_t stride = (uint64_t)gridDim.x * 256;
        for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wave) * 64; w0 < limit; w0 += stride) {
            const uint32_t nvalid = limit - w0 < 64 ? (uint32_t)(limit - w0) : 64u;
            const uint32_t lrow = (uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1;
            const uint32_t seq = (uint32_t)w0 + lrow;
            f(w0, nvalid, seq, entry(seq));
        }
    }
    // The same windows under a per-position test bit(lpos): walk_seq_windows below over this sequence's entries
    template <class B, class T>
    __device__ __forceinline__ void filtered_windows(uint32_t limit, float *lds, int wave, int lane, B &&bit, T &&tile) const;
};
// The windows of a candidate sequence under a per-position test (PartitionSeq::filtered_windows; RowsSeq, kernels_rows.hip): wave
// w of block x takes the 64-position windows (turn * gridDim.x + x) * 4 + w while they begin below `limit`; lane l's position gets
// lpos = entry(seq) and, where it is inside the sequence, bit(lpos, seq) -- called for exactly those positions, once each.  The
// set ones are balloted and compacted through a WindowQueue with lpos as payload; tile(lpos, seq, nvalid) runs whenever 64 are
// queued and once more behind the wave's last window (ONE call site, as in filtered_walk: the chain and the list's offer are
// instantiated once), so a position that fails the test is never loaded.  The lanes behind a last tile's end follow its last
// entry, payload included.
template <class E, class B, class T>
__device__ __forceinline__ void walk_seq_windows(uint32_t limit, float *lds, int wave, int lane, E &&entry, B &&bit, T &&tile) {
    WindowQueue<true> wq;
    wq.cq = reinterpret_cast<uint32_t *>(lds);
    const uint64_t stride = (uint64_t)gridDim.x * 256;
    for (uint64_t w0 = ((uint64_t)blockIdx.x * 4 + wave) * 64;; w0 += stride) {
        const bool last = w0 >= limit;
        QueueTile t;
        if (!last) {
            const uint32_t nvalid = limit - w0 < 64 ? (uint32_t)(limit - w0) : 64u;
            const uint32_t lrow = (uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1;
            const uint32_t seq = (uint32_t)w0 + lrow;
            const uint32_t lpos = entry(seq);
            const bool on = (uint32_t)lane < nvalid && bit(lpos, seq);
            t = wq.push(__ballot(on), w0, lpos, lane);
        } else {
            t = wq.flush(lane);
        }
        if (t.nvalid) {
            const uint32_t lp = (uint32_t)__shfl((int)t.my_x, (int)((uint32_t)lane < t.nvalid ? (uint32_t)lane : t.nvalid - 1), 64);
            tile(lp, t.my_r, t.nvalid);
        }
        if (last) break;
    }
}
template <class B, class T>
__device__ __forceinline__ void PartitionSeq::filtered_windows(uint32_t limit, float *lds, int wave, int lane, B &&bit, T &&tile) const {
    walk_seq_windows(limit, lds, wave, lane, [&](uint32_t seq) { return entry(seq); }, [&](uint32_t lpos, uint32_t) { return bit(lpos); }, tile);
}
// bit p of a position image (a mask's or a key column's validity): a gathered 8-byte load; nullptr: set
__device__ __forceinline__ bool image_bit(const uint64_t *img, uint32_t p) { return !img || ((img[p >> 6] >> (p & 63u)) & 1ull); }

// ------------------------------------------------------------------------------------
// The per-query key test (pqv.h: pqv_key_filter).  KIND 0 (PQV_KEY_EQ): key == lo.  KIND 1 (PQV_KEY_RANGE): lo <= key && key <=
// hi.  KIND 2 (PQV_KEY_IN): the block copies its query's slice vals[lims[q] .. lims[q + 1]) -- never more than KEY_SET_MAX
// values, never anything outside the slice -- into `set_lds` (8 KiB) and passes the block's barrier: EVERY wave must reach
// setup_in, ahead of every early exit that is not block-uniform; a lane's key is then looked up by a halving search whose trip count
// depends on the slice length only.  A slice that is not ascending finds some keys and misses others; every index the search forms
// stays below the slice length.  An empty slice matches nothing: the caller walks nothing (window needs n >= 1).
// ------------------------------------------------------------------------------------
// the key of list position `at`, an i32 column's value widened
__device__ __forceinline__ int64_t load_key_pos(const void *key_pos, bool is_i32, uint64_t at) {
    if (is_i32) return (int64_t) static_cast<const int32_t *>(key_pos)[at];
    return static_cast<const int64_t *>(key_pos)[at];
}

template <int KIND>
struct KeyTest {
    int64_t lo = 0, hi = 0;
    const int64_t *kset = nullptr;
    uint32_t n = 0;         // IN: the values held in kset (block-uniform)

    __device__ __forceinline__ void setup_in(const void *lims, const void *vals, uint32_t q, int64_t *set_lds) {
        const uint64_t s0 = static_cast<const uint64_t *>(lims)[q], s1 = static_cast<const uint64_t *>(lims)[q + 1];
        if (s1 > s0) n = s1 - s0 > (uint64_t)KEY_SET_MAX ? KEY_SET_MAX : (uint32_t)(s1 - s0);
        for (uint32_t i = threadIdx.x; i < n; i += 256) set_lds[i] = static_cast<const int64_t *>(vals)[s0 + i];
        __syncthreads();
        kset = set_lds;
    }
    __device__ __forceinline__ bool empty() const { return KIND == 2 && n == 0; }

    // the 64 bits of the test from position p on: lane l loads key_pos[p + l] (one coalesced 256- / 512-byte read; key_pos is padded
    // by a whole window, so p + lane is always in range), ANDed with the column's validity image where it has one
    __device__ __forceinline__ uint64_t window(const void *key_pos, bool is_i32, const uint64_t *valid_pos, uint64_t p, int lane) const {
        const int64_t kv = load_key_pos(key_pos, is_i32, p + (uint64_t)lane);
        uint64_t win;
        if constexpr (KIND == 0) {
            win = __ballot(kv == lo);
        } else if constexpr (KIND == 1) {
            win = __ballot(lo <= kv && kv <= hi);
        } else {
            uint32_t at = 0;
            for (uint32_t span = n; span > 1;) {                // (wave-uniform trip count; at + half < n)
                const uint32_t half = span >> 1;
                if (kset[at + half] <= kv) at += half;
                span -= half;
            }
            win = __ballot(kset[at] == kv);
        }
        if (valid_pos) win &= image_window(valid_pos, p);
        return win;
    }
};

// The test of a distinct / grouped call's filter (GroupFilterArgs), set up once per block: PQV_KEY_EQ runs as the range [a[q], a[q]].
__device__ __forceinline__ void group_filter_bounds(const GroupFilterArgs &fa, uint32_t q, KeyTest<1> &kt) {
    kt.lo = static_cast<const int64_t *>(fa.a)[q];
    kt.hi = fa.kind == 0 ? kt.lo : static_cast<const int64_t *>(fa.b)[q];
}

// ------------------------------------------------------------------------------------
// The k groups pass 1 of a grouped call named (launch_group_set's outputs), staged once per block in LDS beside the tile area:
// 5 KB, GROUPED_SET_MAX i64 values ascending and their u16 slots.  stage() ends WITHOUT a barrier: the caller passes one before
// the first lookup.  lookup: a branch-free binary search over full i64 values.
// ------------------------------------------------------------------------------------
struct GroupSet {
    int64_t *v;
    uint16_t *s;
    uint32_t n;

    __device__ __forceinline__ void stage(const GroupedArgs &ga, uint32_t q, int64_t *set_v, uint16_t *set_s) {
        v = set_v; s = set_s;
        n = ga.n_found[q];
        if (n > ga.k) n = ga.k;
        for (uint32_t i = threadIdx.x; i < n; i += 256) {
            set_v[i] = ga.set_keys[(uint64_t)q * ga.k + i];
            set_s[i] = (uint16_t)ga.set_slot[(uint64_t)q * ga.k + i];
        }
    }
    // is kv one of the groups (n >= 1), and its slot
    __device__ __forceinline__ bool lookup(int64_t kv, uint32_t &slot) const {
        uint32_t at = 0;
        for (uint32_t span = n; span > 1;) {            // (wave-uniform trip count; at + half - 1 < n)
            const uint32_t half = span >> 1;
            if (v[at + half - 1] < kv) at += half;
            span -= half;
        }
        slot = s[at];
        return v[at] == kv;
    }
};

// ------------------------------------------------------------------------------------
// Outputs.
// ------------------------------------------------------------------------------------
// STREAM_RANGE: the wave's hits go to the query's segment in one block: ballot, rank from mbcnt, one atomicAdd per wave
__device__ __forceinline__ void emit_range_hit(const StreamArgs &a, uint32_t q, bool hit, uint64_t key, uint32_t my_srow, int lane) {
    const uint64_t m = __ballot(hit);
    if (m) {
        uint32_t base = 0;
        if (lane == 0) base = atomicAdd(a.hit_cnt + q, (uint32_t)__popcll(m));
        base = (uint32_t)__shfl((int)base, 0, 64);
        const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (hit) {
            const uint64_t o = range_seg_base(a.seg_off, a.seg_stride, q) + base + rank;
            a.hit_keys[o] = key;
            a.hit_vals[o] = my_srow;
        }
    }
}
// a hit of the L2 forms: out = (sqrt_out 1 ? sqrt(d2) : 2 ? 0.5 d2 (PQV_COSINE) : d2) <= radius (a NaN distance never compares true)
__device__ __forceinline__ void emit_l2_range_hit(const StreamArgs &a, uint32_t q, bool valid, float sum, uint64_t pos, uint32_t my_srow, int lane) {
    const float outv = a.sqrt_out == 1 ? sqrt_f32_ieee(sum) : a.sqrt_out == 2 ? 0.5f * sum : sum;
    emit_range_hit(a, q, valid && outv <= a.radius, l2_key(sum, pos), my_srow, lane);
}

// the wave's partial list: index among the query's n_part = nprobe * blocks_per_list * 4 lists, and where a list of `width` begins
__device__ __forceinline__ uint32_t partial_index(const StreamArgs &a, uint32_t j, int wave) { return (j * a.blocks_per_list + blockIdx.x) * 4 + wave; }
__device__ __forceinline__ uint64_t partial_base(const StreamArgs &a, uint32_t q, uint32_t j, int wave, uint32_t width) {
    return ((uint64_t)q * (a.nprobe * a.blocks_per_list * 4) + partial_index(a, j, wave)) * width;
}
// the first `count` entries of a wave-distributed list (element e in register e / 64 of lane e % 64) to part_keys / part_vals
// [nq][n_part][width]; extra(o, s): what else goes with entry (register s of this lane) at offset o
template <int S, class F>
__device__ __forceinline__ void write_partial_lists(uint64_t *part_keys, uint32_t *part_vals, uint64_t base, uint32_t count, int lane,
                                                    const uint64_t (&key)[S], const uint32_t (&val)[S], F &&extra) {
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        if (e < count) {
            part_keys[base + e] = key[s];
            part_vals[base + e] = val[s];
            extra(base + e, s);
        }
    }
}
template <int S>
__device__ __forceinline__ void write_partial_lists(uint64_t *part_keys, uint32_t *part_vals, uint64_t base, uint32_t count, int lane,
                                                    const uint64_t (&key)[S], const uint32_t (&val)[S]) {
    write_partial_lists<S>(part_keys, part_vals, base, count, lane, key, val, [](uint64_t, int) {});
}

// ------------------------------------------------------------------------------------
// What the distinct and grouped forms share with their filtered twins (TK: the wave's list, wave_group_lists.hpp).
// ------------------------------------------------------------------------------------
// the bits every window of theirs starts from: the group column's validity image ANDed with the shared mask's, all ones where
// the call has neither, clipped to the range: a NULL-key row belongs to no group and is never read
__device__ __forceinline__ uint64_t group_images_window(const uint64_t *valid_pos, const uint64_t *bits, uint64_t p, uint64_t clip) {
    uint64_t win = clip;
    if (valid_pos) win &= image_window(valid_pos, p);
    if (bits) win &= image_window(bits, p);
    return win;
}

// a distinct tile: lane l loads its row's group value key_pos[lbeg + my_r] (one gathered 4- / 8-byte load per evaluated row -- a
// candidate position, below the image's n_pos -- issued ahead of the chain) and offers (key, storage row, group)
template <int CG, bool SEQ, bool ALIGNED, int GW, class TK>
__device__ __forceinline__ void distinct_tile(const StreamArgs &a, const void *key_pos, const WalkRange &w, const QueueTile &t, float *lds,
                                              const float *qv, int lane, TK &tk) {
    const uint64_t lpos = w.lbeg + t.my_r;
    const uint32_t my_srow = storage_row(a, lpos);
    uint32_t mygrp[GW];
    if constexpr (GW == 1) {
        mygrp[0] = static_cast<const uint32_t *>(key_pos)[lpos];
    } else {
        const uint64_t gv = static_cast<const uint64_t *>(key_pos)[lpos];
        mygrp[0] = (uint32_t)gv; mygrp[1] = (uint32_t)(gv >> 32);
    }
    const float sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, t.nvalid, lane);
    const bool valid = (uint32_t)lane < t.nvalid;           // (pos < lim by the clamp of the walk)
    tk.offer(valid ? l2_key(sum, w.cbase + t.my_r) : KEY_EMPTY, my_srow, mygrp, a.k, lane);
}
// ... and its list: part_keys / part_vals / part_grp [nq][n_part][k], group values widened to i64
template <int S, int GW, class TK>
__device__ __forceinline__ void write_distinct_lists(const StreamArgs &a, int64_t *part_grp, uint64_t base, int lane, const TK &tk) {
    write_partial_lists<S>(a.part_keys, a.part_vals, base, a.k, lane, tk.key, tk.val, [&](uint64_t o, int s) {
        if constexpr (GW == 1) part_grp[o] = (int64_t)(int32_t)tk.grp[s][0];
        else part_grp[o] = (int64_t)(((uint64_t)tk.grp[s][1] << 32) | (uint64_t)tk.grp[s][0]);
    });
}

// a rank at or beyond the query's limit (DistinctArgs::rank_limit): the wave's list goes out EMPTY, as init() leaves it
__device__ __forceinline__ void write_empty_distinct_list(const StreamArgs &a, int64_t *part_grp, uint64_t base, int lane) {
    for (uint32_t e = (uint32_t)lane; e < a.k; e += 64) {
        a.part_keys[base + e] = KEY_EMPTY;
        a.part_vals[base + e] = 0xFFFFFFFFu;
        part_grp[base + e] = 0;
    }
}

// grouped: MEMBERSHIP of a window's positions in the query's k groups -- lane l reads key_pos[p + l] (one coalesced window, as
// the key test reads it; p + lane < the image's n_words * 64) and looks it up; slot: lane l's slot where it is a member
__device__ __forceinline__ uint64_t group_member_window(const GroupSet &gs, const void *key_pos, bool is_i32, uint64_t p, int lane, uint32_t &slot) {
    return __ballot(gs.lookup(load_key_pos(key_pos, is_i32, p + (uint64_t)lane), slot));
}
// a grouped tile: the slot travelled through the queue beside the list offset; lane l offers (key, storage row, slot)
template <int CG, bool SEQ, bool ALIGNED, class TK>
__device__ __forceinline__ void grouped_tile(const StreamArgs &a, uint32_t group_size, const WalkRange &w, const QueueTile &t, float *lds,
                                             const float *qv, int lane, TK &tk) {
    const uint32_t my_srow = storage_row(a, w.lbeg + t.my_r);
    const float sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, t.nvalid, lane);
    const bool valid = (uint32_t)lane < t.nvalid;           // (pos < lim by the clamp of the walk)
    tk.offer(valid ? l2_key(sum, w.cbase + t.my_r) : KEY_EMPTY, my_srow, t.my_x, group_size, lane);
}
// ... and its list: the filled part to part_keys / part_vals / part_slot [nq][n_part][km], the length to part_cnt [nq][n_part] --
// most waves of a call meet a handful of members, and the fold reads what was written, not km entries per wave
template <int S, class TK>
__device__ __forceinline__ void write_grouped_lists(const StreamArgs &a, const GroupedArgs &ga, uint32_t q, uint32_t j, int wave, int lane, const TK &tk) {
    write_partial_lists<S>(ga.part_keys, ga.part_vals, partial_base(a, q, j, wave, ga.km), tk.n, lane, tk.key, tk.val,     // (n <= km)
                           [&](uint64_t o, int s) { ga.part_slot[o] = tk.slot[s]; });
    if (lane == 0) ga.part_cnt[partial_base(a, q, j, wave, 1)] = tk.n;
}

// ------------------------------------------------------------------------------------
// Host: the chunk choice of every launcher (the chain order does not depend on it).  f(CG, SEQ, ALIGNED) gets the three as
// integral_constants: PQV_L2SQ_SEQ (metric 1) -> CG 16, four squares; an unaligned dimension -> CG 32; a dimension of whole
// 64-group chunks -> CG 64; else CG 32.  SEQ_OK = false: the form has no SEQ chain (dot).  WIDE_OK = false: no CG 64 form.
// ------------------------------------------------------------------------------------
template <bool SEQ_OK = true, bool WIDE_OK = true, class F>
static inline hipError_t dispatch_chunk(uint32_t dim, int metric, F &&f) {
    using std::false_type;
    using std::true_type;
    const bool aligned = (dim % 4) == 0;
    const uint32_t G = dim / 4;
    if constexpr (SEQ_OK) {
        if (metric == 1) {
            return aligned ? f(std::integral_constant<int, 16>{}, true_type{}, true_type{})
                           : f(std::integral_constant<int, 16>{}, true_type{}, false_type{});
        }
    }
    if (!aligned) return f(std::integral_constant<int, 32>{}, false_type{}, false_type{});
    if constexpr (WIDE_OK) {
        if (G >= 64 && G % 64 == 0) return f(std::integral_constant<int, 64>{}, false_type{}, true_type{});
    }
    return f(std::integral_constant<int, 32>{}, false_type{}, true_type{});
}

// Host: what every walk of a key partition's candidate sequences (PartitionSeq) asks of its arguments: the partition's positions, the
// span kernel's outputs for the filter's kind, and a (B, nq) grid; each launcher adds the checks of its own outputs.
static inline bool partition_walk_ok(const StreamArgs &a, const PartitionArgs &pa) {
    if (!pa.pos || !pa.span_beg || !pa.n_cand || (pa.kind == 2 && (!pa.span_end || !pa.n_span)) || pa.kind > 2) return false;
    return a.nprobe == 1 && a.blocks_per_list != 0 && a.blocks_per_list <= 0xFFFFu && a.nq <= 0xFFFFu;
}

// Host: the list length choice of every launcher.  f(S) gets the 64-entry slots a lane's sorted list takes as an integral_constant:
// k <= 64 -> 1, <= 256 -> 4, <= 1024 -> 16; the kernels hold no longer list.
template <class F>
static inline hipError_t dispatch_list_slots(uint32_t k, F &&f) {
    if (k <= 64) return f(std::integral_constant<int, 1>{});
    if (k <= 256) return f(std::integral_constant<int, 4>{});
    if (k <= 1024) return f(std::integral_constant<int, 16>{});
    return hipErrorInvalidValue;
}

}  // namespace pqv

#endif  // PQV_STREAM_WALK_HPP
