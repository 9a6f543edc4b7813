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
#include "wave_group_lists.hpp"

namespace pqv {

// The query's test, set up once per block.  IN: the block copies b[a[q] .. a[q + 1]) -- at most KEY_SET_MAX values, never anything
// outside the slice -- into `set_lds` and passes the barrier; returns the slice length.  Else lo / hi are the inclusive bounds.
template <bool IN>
__device__ __forceinline__ uint32_t group_filter_setup(const GroupFilterArgs &fa, uint32_t q, int64_t *set_lds, int64_t &lo, int64_t &hi) {
    uint32_t n = 0;
    if constexpr (IN) {
        const uint64_t s0 = static_cast<const uint64_t *>(fa.a)[q], s1 = static_cast<const uint64_t *>(fa.a)[q + 1];
        if (s1 > s0) n = s1 - s0 > (uint64_t)KEY_SET_MAX ? KEY_SET_MAX : (uint32_t)(s1 - s0);
        for (uint32_t i = threadIdx.x; i < n; i += 256) set_lds[i] = static_cast<const int64_t *>(fa.b)[s0 + i];
        __syncthreads();
    } else {
        lo = static_cast<const int64_t *>(fa.a)[q];
        hi = fa.kind == 0 ? lo : static_cast<const int64_t *>(fa.b)[q];
    }
    return n;
}

// the 64 bits of the filter from position p on (validity included); kset_n >= 1 for IN
template <bool IN>
__device__ __forceinline__ uint64_t group_filter_window(const GroupFilterArgs &fa, uint64_t p, int lane, const int64_t *kset, uint32_t kset_n,
                                                        int64_t lo, int64_t hi) {
    // (key_pos is padded by a whole window: p + lane is always in range; positions at or beyond the range's end are clipped by the caller)
    int64_t kv;
    if (fa.elem_size == 4) kv = (int64_t) static_cast<const int32_t *>(fa.key_pos)[p + (uint64_t)lane];
    else kv = static_cast<const int64_t *>(fa.key_pos)[p + (uint64_t)lane];
    uint64_t win;
    if constexpr (IN) {
        uint32_t at = 0;
        for (uint32_t span = kset_n; span > 1;) {           // (wave-uniform trip count; at + half < kset_n)
            const uint32_t half = span >> 1;
            if (kset[at + half] <= kv) at += half;
            span -= half;
        }
        win = __ballot(kset[at] == kv);
    } else {
        win = __ballot(lo <= kv && kv <= hi);
    }
    if (fa.valid_pos) win &= image_window(fa.valid_pos, p);
    return win;
}

// ------------------------------------------------------------------------------------
// distinct_filter_stream_kernel
//
// distinct_stream_kernel with one more source of a window's bits.  Grid (row block, probe rank, query), 4 independent waves per
// block, the cap / pair_end / max_pos clamp BEFORE any filter, the queue in a register and the compaction through the idle tile
// area, the chain arithmetic element for element, keys (d2 bits << 32) | (u32)(cbase + position), the group value gathered per
// evaluated row, the statistics words, and part_keys / part_vals / part_grp [nq][n_part][k].
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW, bool IN>
__global__ __launch_bounds__(256) void distinct_filter_stream_kernel(const StreamArgs a, const DistinctArgs da, const GroupFilterArgs fa) {
    constexpr int RPI = 64 / CG;        // rows per load instruction
    constexpr int NI = CG;              // load instructions per 64-row tile
    constexpr int EPL = SEQ ? 4 : 1;    // LDS values per lane item
    constexpr int LROWS = CG * EPL;     // chain length per chunk
    constexpr int NB = 8;               // loads in flight per lane
    static_assert(NI % NB == 0, "NI must be a multiple of NB");
    static_assert(LROWS * 64 >= 128, "the compaction needs 128 words of the tile area");

    __shared__ float lds_all[4 * LROWS * 64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * (LROWS * 64);
    uint32_t *cq = reinterpret_cast<uint32_t *>(lds);          // compaction scratch: 128 entries
#define LDS_AT(e, r) lds[(e) * 64 + ((r) ^ ((e) & 63))]

    const uint32_t q = blockIdx.z, j = blockIdx.y;
    // the query's test (block-uniform; IN: every wave of the block passes the barrier before it looks at its range)
    int64_t flo = 0, fhi = 0;
    const int64_t *kset = nullptr;
    uint32_t kset_n = 0;
    if constexpr (IN) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        kset_n = group_filter_setup<true>(fa, q, set_lds, flo, fhi);
        kset = set_lds;
    } else {
        group_filter_setup<false>(fa, q, nullptr, flo, fhi);
    }

    const uint32_t c = a.probe[(uint64_t)q * a.nprobe + j];
    const uint64_t lbeg = a.list_off[c], lend = a.list_off[c + 1];
    const uint64_t cbase = a.cand_base[(uint64_t)q * a.nprobe + j];
    const uint64_t lim = a.pair_end ? a.pair_end[(uint64_t)q * a.nprobe + j] : a.max_pos;
    uint64_t len = lend - lbeg;
    // positions at or beyond the cap are no candidates: the walk ends there (their bits are never looked at)
    const uint64_t room = lim > cbase ? lim - cbase : 0;
    if (len > room) len = room;
    const uint64_t wrows = a.rows_per_block / 4;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.rows_per_block + (uint64_t)wave * wrows;
    uint64_t r1 = r0 + wrows;
    if (r1 > len) r1 = len;
    if (IN && kset_n == 0) r1 = 0;      // (nothing matches: no window is read)

#ifdef PQV_PROFILE_PHASES
    unsigned long long *st = da.stats;
#else
    unsigned long long *st = da.stats ? da.stats + 8 + 16 * (q % STATS_SLOTS) : nullptr;
#endif
    if (da.n_cand && st && blockIdx.x == 0 && j == 0 && threadIdx.x == 0) atomicAdd(&st[2], (unsigned long long)da.n_cand[q]);

    const uint32_t dim = a.dim;
    const uint32_t G = dim >> 2;
    const uint32_t tail = dim & 3u;
    const float *qv = a.queries + (uint64_t)q * dim;
    const int g_in = lane % CG;      // my float4 group inside a chunk
    const int row_in = lane / CG;    // my row inside a load instruction

    WaveDistinctTopk<S, GW> tk;
    tk.init();

    uint32_t pend = 0;      // queue entry `lane` (a list offset, < 2^32 as every candidate position), meaningful for lane < qn
    uint32_t qn = 0;        // queued entries, < 64 between two windows (wave-uniform)
    uint32_t n_eval = 0;    // rows this wave evaluated (wave-uniform)
    for (uint64_t w0 = r0;; w0 += 64) {
        const bool flush = w0 >= r1;        // past the range: what is left in the queue is the last tile
        uint32_t nvalid = 0;                // rows of the chain tile this turn runs (0: none)
        uint32_t my_r = 0;                  // list offset of tile row `lane`
        if (!flush) {
            const uint64_t p = lbeg + w0;
            uint64_t win = ~0ull;
            if (da.valid_pos) win &= image_window(da.valid_pos, p);
            if (da.bits) win &= image_window(da.bits, p);
            if (r1 - w0 < 64) win &= (1ull << (r1 - w0)) - 1ull;
            if (win == 0) continue;
            win &= group_filter_window<IN>(fa, p, lane, kset, kset_n, flo, fhi);
            const uint32_t cnt = (uint32_t)__popcll(win);
            if (cnt == 0) continue;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(win >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)win, 0u));
            if ((uint32_t)lane < qn) cq[lane] = pend;
            if ((win >> lane) & 1ull) cq[qn + rank] = (uint32_t)(w0 + (uint64_t)lane);
            wave_lds_fence();
            const uint32_t total = qn + cnt;                   // <= 127
            const uint32_t first = cq[lane];
            const uint32_t over = cq[64 + lane];
            wave_lds_fence();
            if (total >= 64) {
                my_r = first; nvalid = 64u;
                pend = over; qn = total - 64;
            } else {
                pend = first; qn = total;
            }
        } else if (qn) {
            const uint32_t last = (uint32_t)__shfl((int)pend, (int)(qn - 1), 64);
            my_r = (uint32_t)lane < qn ? pend : last;         // (clamped: every address in range)
            nvalid = qn; qn = 0;
        }
        if (nvalid) {
            n_eval += nvalid;
            const uint64_t lpos = lbeg + my_r;
            const uint32_t my_srow = a.row_of ? a.row_of[lpos] : (uint32_t)lpos;
            // my row's group value (lpos < the image's n_pos: a candidate position), back by the end of the chain
            uint32_t mygrp[GW];
            if constexpr (GW == 1) {
                mygrp[0] = static_cast<const uint32_t *>(da.key_pos)[lpos];
            } else {
                const uint64_t gv = static_cast<const uint64_t *>(da.key_pos)[lpos];
                mygrp[0] = (uint32_t)gv; mygrp[1] = (uint32_t)(gv >> 32);
            }

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
                        const float d0 = qq.x - x[u].x, d1 = qq.y - x[u].y;
                        const float d2 = qq.z - x[u].z, d3 = qq.w - x[u].w;
                        if constexpr (SEQ) {
                            if (gvalid) {
                                LDS_AT(g_in * 4 + 0, rr) = d0 * d0;
                                LDS_AT(g_in * 4 + 1, rr) = d1 * d1;
                                LDS_AT(g_in * 4 + 2, rr) = d2 * d2;
                                LDS_AT(g_in * 4 + 3, rr) = d3 * d3;
                            }
                        } else {
                            float t = d0 * d0 + d1 * d1;
                            t = t + d2 * d2;
                            t = t + d3 * d3;
                            if (gvalid) LDS_AT(g_in, rr) = t;
                        }
                    }
                }
                wave_lds_fence();
                const uint32_t nchain = ng * EPL;
                uint32_t e = 0;
                for (; e + 8 <= nchain; e += 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = LDS_AT(e + u, lane);
#pragma unroll
                    for (int u = 0; u < 8; ++u) sum = sum + v[u];
                }
                for (; e < nchain; ++e) sum = sum + LDS_AT(e, lane);
                wave_lds_fence();
            }
            if (tail) {  // scalar tail of squared_l2_distance
                const float *xr = a.mat + (uint64_t)my_srow * dim + (uint64_t)G * 4;
                const float *qt = qv + (uint64_t)G * 4;
                for (uint32_t e = 0; e < tail; ++e) {
                    const float d = qt[e] - xr[e];
                    sum = sum + d * d;
                }
            }

            const uint64_t pos = cbase + my_r;
            const bool valid = (uint32_t)lane < nvalid;           // (pos < lim by the clamp of the walk)
            const uint64_t mykey = valid ? (((uint64_t)__float_as_uint(sum) << 32) | (uint64_t)(uint32_t)pos) : KEY_EMPTY;
            tk.offer(mykey, my_srow, mygrp, a.k, lane);
        }
        if (flush) break;
    }
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    const uint32_t n_part = a.nprobe * a.blocks_per_list * 4;
    const uint32_t pi = (j * a.blocks_per_list + blockIdx.x) * 4 + wave;
    const uint64_t base = ((uint64_t)q * n_part + pi) * a.k;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        if (e < a.k) {
            a.part_keys[base + e] = tk.key[s];
            a.part_vals[base + e] = tk.val[s];
            if constexpr (GW == 1) da.part_grp[base + e] = (int64_t)(int32_t)tk.grp[s][0];
            else da.part_grp[base + e] = (int64_t)(((uint64_t)tk.grp[s][1] << 32) | (uint64_t)tk.grp[s][0]);
        }
    }
}

template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
static hipError_t launch_distinct_filter_t(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s) {
    dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
    if (fa.kind == 2) hipLaunchKernelGGL((distinct_filter_stream_kernel<CG, S, SEQ, ALIGNED, GW, true>), grid, dim3(256), 0, s, a, da, fa);
    else hipLaunchKernelGGL((distinct_filter_stream_kernel<CG, S, SEQ, ALIGNED, GW, false>), grid, dim3(256), 0, s, a, da, fa);
    return hipGetLastError();
}

// the chunk choice of launch_stream (the chain order does not depend on it)
template <int S, int GW>
static hipError_t launch_distinct_filter_s(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s) {
    const bool aligned = (a.dim % 4) == 0;
    const uint32_t G = a.dim / 4;
    if (a.metric == 1) {
        return aligned ? launch_distinct_filter_t<16, S, true, true, GW>(a, da, fa, s) : launch_distinct_filter_t<16, S, true, false, GW>(a, da, fa, s);
    }
    if (!aligned) return launch_distinct_filter_t<32, S, false, false, GW>(a, da, fa, s);
    if (G >= 64 && G % 64 == 0) return launch_distinct_filter_t<64, S, false, true, GW>(a, da, fa, s);
    return launch_distinct_filter_t<32, S, false, true, GW>(a, da, fa, s);
}

template <int GW>
static hipError_t launch_distinct_filter_w(const StreamArgs &a, const DistinctArgs &da, const GroupFilterArgs &fa, hipStream_t s) {
    if (a.k <= 64) return launch_distinct_filter_s<1, GW>(a, da, fa, s);
    if (a.k <= 256) return launch_distinct_filter_s<4, GW>(a, da, fa, s);
    if (a.k <= 1024) return launch_distinct_filter_s<16, GW>(a, da, fa, s);
    return hipErrorInvalidValue;
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
    constexpr int RPI = 64 / CG;        // rows per load instruction
    constexpr int NI = CG;              // load instructions per 64-row tile
    constexpr int EPL = SEQ ? 4 : 1;    // LDS values per lane item
    constexpr int LROWS = CG * EPL;     // chain length per chunk
    constexpr int NB = 8;               // loads in flight per lane
    static_assert(NI % NB == 0, "NI must be a multiple of NB");
    static_assert(LROWS * 64 >= 256, "the compaction needs 256 words of the tile area");

    __shared__ float lds_all[4 * LROWS * 64];
    __shared__ int64_t set_v[GROUPED_SET_MAX];
    __shared__ uint16_t set_s[GROUPED_SET_MAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * (LROWS * 64);
    uint32_t *cq = reinterpret_cast<uint32_t *>(lds);          // compaction scratch: 128 list offsets, then 128 slots
    uint32_t *cs = cq + 128;
#define LDS_AT(e, r) lds[(e) * 64 + ((r) ^ ((e) & 63))]

    const uint32_t q = blockIdx.z, j = blockIdx.y;
    // the query's set and test (block-uniform; every wave of the block passes the barriers before it looks at its range)
    uint32_t set_n = ga.n_found[q];
    if (set_n > ga.k) set_n = ga.k;
    for (uint32_t i = threadIdx.x; i < set_n; i += 256) {
        set_v[i] = ga.set_keys[(uint64_t)q * ga.k + i];
        set_s[i] = (uint16_t)ga.set_slot[(uint64_t)q * ga.k + i];
    }
    int64_t flo = 0, fhi = 0;
    const int64_t *kset = nullptr;
    uint32_t kset_n = 0;
    if constexpr (IN) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        kset_n = group_filter_setup<true>(fa, q, set_lds, flo, fhi);      // (its barrier covers set_v / set_s too)
        kset = set_lds;
    } else {
        group_filter_setup<false>(fa, q, nullptr, flo, fhi);
        __syncthreads();
    }

    const uint32_t c = a.probe[(uint64_t)q * a.nprobe + j];
    const uint64_t lbeg = a.list_off[c], lend = a.list_off[c + 1];
    const uint64_t cbase = a.cand_base[(uint64_t)q * a.nprobe + j];
    const uint64_t lim = a.pair_end ? a.pair_end[(uint64_t)q * a.nprobe + j] : a.max_pos;
    uint64_t len = lend - lbeg;
    // positions at or beyond the cap are no candidates: the walk ends there (their bits are never looked at)
    const uint64_t room = lim > cbase ? lim - cbase : 0;
    if (len > room) len = room;
    const uint64_t wrows = a.rows_per_block / 4;
    const uint64_t r0 = (uint64_t)blockIdx.x * a.rows_per_block + (uint64_t)wave * wrows;
    uint64_t r1 = r0 + wrows;
    if (r1 > len) r1 = len;
    if (set_n == 0) r1 = 0;             // no group: nothing to walk, an empty list is written
    if (IN && kset_n == 0) r1 = 0;      // (cannot be with set_n > 0: a group of pass 1 has a passing row)

#ifdef PQV_PROFILE_PHASES
    unsigned long long *st = ga.stats;
#else
    unsigned long long *st = ga.stats ? ga.stats + 8 + 16 * (q % STATS_SLOTS) : nullptr;
#endif

    const uint32_t dim = a.dim;
    const uint32_t G = dim >> 2;
    const uint32_t tail = dim & 3u;
    const float *qv = a.queries + (uint64_t)q * dim;
    const int g_in = lane % CG;      // my float4 group inside a chunk
    const int row_in = lane / CG;    // my row inside a load instruction

    WaveGroupedTopk<S> tk;
    tk.init();

    uint32_t pend = 0;      // queue entry `lane` (a list offset, < 2^32 as every candidate position), meaningful for lane < qn
    uint32_t pend_s = 0;    // ... and its slot
    uint32_t qn = 0;        // queued entries, < 64 between two windows (wave-uniform)
    uint32_t n_eval = 0;    // rows this wave evaluated (wave-uniform)
    for (uint64_t w0 = r0;; w0 += 64) {
        const bool flush = w0 >= r1;        // past the range: what is left in the queue is the last tile
        uint32_t nvalid = 0;                // rows of the chain tile this turn runs (0: none)
        uint32_t my_r = 0;                  // list offset of tile row `lane`
        uint32_t my_slot = 0;               // ... and its slot
        if (!flush) {
            const uint64_t p = lbeg + w0;
            uint64_t win = ~0ull;
            if (ga.valid_pos) win &= image_window(ga.valid_pos, p);
            if (ga.bits) win &= image_window(ga.bits, p);
            if (r1 - w0 < 64) win &= (1ull << (r1 - w0)) - 1ull;
            if (win == 0) continue;
            win &= group_filter_window<IN>(fa, p, lane, kset, kset_n, flo, fhi);
            if (win == 0) continue;
            // membership: my position's group value (p + lane < the image's n_words * 64) against the sorted set
            int64_t kv;
            if (ga.elem_size == 4) kv = (int64_t) static_cast<const int32_t *>(ga.key_pos)[p + (uint64_t)lane];
            else kv = static_cast<const int64_t *>(ga.key_pos)[p + (uint64_t)lane];
            uint32_t at = 0;
            for (uint32_t span = set_n; span > 1;) {            // (wave-uniform trip count; at + half - 1 < set_n)
                const uint32_t half = span >> 1;
                if (set_v[at + half - 1] < kv) at += half;
                span -= half;
            }
            const bool member = set_v[at] == kv;
            const uint32_t slot_w = set_s[at];
            win &= __ballot(member);
            const uint32_t cnt = (uint32_t)__popcll(win);
            if (cnt == 0) continue;
            const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(win >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)win, 0u));
            if ((uint32_t)lane < qn) { cq[lane] = pend; cs[lane] = pend_s; }
            if ((win >> lane) & 1ull) { cq[qn + rank] = (uint32_t)(w0 + (uint64_t)lane); cs[qn + rank] = slot_w; }
            wave_lds_fence();
            const uint32_t total = qn + cnt;                   // <= 127
            const uint32_t first = cq[lane], first_s = cs[lane];
            const uint32_t over = cq[64 + lane], over_s = cs[64 + lane];
            wave_lds_fence();
            if (total >= 64) {
                my_r = first; my_slot = first_s; nvalid = 64u;
                pend = over; pend_s = over_s; qn = total - 64;
            } else {
                pend = first; pend_s = first_s; qn = total;
            }
        } else if (qn) {
            const uint32_t last = (uint32_t)__shfl((int)pend, (int)(qn - 1), 64);
            my_r = (uint32_t)lane < qn ? pend : last;         // (clamped: every address in range)
            my_slot = pend_s;
            nvalid = qn; qn = 0;
        }
        if (nvalid) {
            n_eval += nvalid;
            const uint64_t lpos = lbeg + my_r;
            const uint32_t my_srow = a.row_of ? a.row_of[lpos] : (uint32_t)lpos;

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
                        const float d0 = qq.x - x[u].x, d1 = qq.y - x[u].y;
                        const float d2 = qq.z - x[u].z, d3 = qq.w - x[u].w;
                        if constexpr (SEQ) {
                            if (gvalid) {
                                LDS_AT(g_in * 4 + 0, rr) = d0 * d0;
                                LDS_AT(g_in * 4 + 1, rr) = d1 * d1;
                                LDS_AT(g_in * 4 + 2, rr) = d2 * d2;
                                LDS_AT(g_in * 4 + 3, rr) = d3 * d3;
                            }
                        } else {
                            float t = d0 * d0 + d1 * d1;
                            t = t + d2 * d2;
                            t = t + d3 * d3;
                            if (gvalid) LDS_AT(g_in, rr) = t;
                        }
                    }
                }
                wave_lds_fence();
                const uint32_t nchain = ng * EPL;
                uint32_t e = 0;
                for (; e + 8 <= nchain; e += 8) {
                    float v[8];
#pragma unroll
                    for (int u = 0; u < 8; ++u) v[u] = LDS_AT(e + u, lane);
#pragma unroll
                    for (int u = 0; u < 8; ++u) sum = sum + v[u];
                }
                for (; e < nchain; ++e) sum = sum + LDS_AT(e, lane);
                wave_lds_fence();
            }
            if (tail) {  // scalar tail of squared_l2_distance
                const float *xr = a.mat + (uint64_t)my_srow * dim + (uint64_t)G * 4;
                const float *qt = qv + (uint64_t)G * 4;
                for (uint32_t e = 0; e < tail; ++e) {
                    const float d = qt[e] - xr[e];
                    sum = sum + d * d;
                }
            }

            const uint64_t pos = cbase + my_r;
            const bool valid = (uint32_t)lane < nvalid;           // (pos < lim by the clamp of the walk)
            const uint64_t mykey = valid ? (((uint64_t)__float_as_uint(sum) << 32) | (uint64_t)(uint32_t)pos) : KEY_EMPTY;
            tk.offer(mykey, my_srow, my_slot, ga.group_size, lane);
        }
        if (flush) break;
    }
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    const uint32_t n_part = a.nprobe * a.blocks_per_list * 4;
    const uint32_t pi = (j * a.blocks_per_list + blockIdx.x) * 4 + wave;
    const uint64_t base = ((uint64_t)q * n_part + pi) * ga.km;
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        if (e < tk.n) {                                         // (n <= km)
            ga.part_keys[base + e] = tk.key[s];
            ga.part_vals[base + e] = tk.val[s];
            ga.part_slot[base + e] = tk.slot[s];
        }
    }
    if (lane == 0) ga.part_cnt[(uint64_t)q * n_part + pi] = tk.n;
}

#undef LDS_AT

template <int CG, int S, bool SEQ, bool ALIGNED>
static hipError_t launch_grouped_filter_t(const StreamArgs &a, const GroupedArgs &ga, const GroupFilterArgs &fa, hipStream_t s) {
    dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
    if (fa.kind == 2) hipLaunchKernelGGL((grouped_filter_stream_kernel<CG, S, SEQ, ALIGNED, true>), grid, dim3(256), 0, s, a, ga, fa);
    else hipLaunchKernelGGL((grouped_filter_stream_kernel<CG, S, SEQ, ALIGNED, false>), grid, dim3(256), 0, s, a, ga, fa);
    return hipGetLastError();
}

// the chunk choice of launch_stream (the chain order does not depend on it)
template <int S>
static hipError_t launch_grouped_filter_s(const StreamArgs &a, const GroupedArgs &ga, const GroupFilterArgs &fa, hipStream_t s) {
    const bool aligned = (a.dim % 4) == 0;
    const uint32_t G = a.dim / 4;
    if (a.metric == 1) {
        return aligned ? launch_grouped_filter_t<16, S, true, true>(a, ga, fa, s) : launch_grouped_filter_t<16, S, true, false>(a, ga, fa, s);
    }
    if (!aligned) return launch_grouped_filter_t<32, S, false, false>(a, ga, fa, s);
    if (G >= 64 && G % 64 == 0) return launch_grouped_filter_t<64, S, false, true>(a, ga, fa, s);
    return launch_grouped_filter_t<32, S, false, true>(a, ga, fa, s);
}

hipError_t launch_grouped_filter_stream(const StreamArgs &a, const GroupedArgs &ga, const GroupFilterArgs &fa, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base || !ga.part_keys || !ga.part_vals || !ga.part_slot || !ga.part_cnt) return hipErrorInvalidValue;
    if (!ga.key_pos || !ga.set_keys || !ga.set_slot || !ga.n_found) return hipErrorInvalidValue;
    // k * group_size <= 1024 with group_size >= 2 (one row per group is the distinct call), hence k <= GROUPED_SET_MAX
    if (ga.k == 0 || ga.group_size < 2 || (uint64_t)ga.k * ga.group_size != ga.km || ga.km > 1024 || ga.k > GROUPED_SET_MAX) return hipErrorInvalidValue;
    if (ga.elem_size != 4 && ga.elem_size != 8) return hipErrorInvalidValue;
    if (!group_filter_args_ok(fa)) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0 || a.nprobe == 0) return hipSuccess;
    if (ga.km <= 64) return launch_grouped_filter_s<1>(a, ga, fa, s);
    if (ga.km <= 256) return launch_grouped_filter_s<4>(a, ga, fa, s);
    return launch_grouped_filter_s<16>(a, ga, fa, s);
}

}  // namespace pqv
