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
#include "wave_group_lists.hpp"

namespace pqv {

// WaveDistinctTopk<S, GW>: wave_group_lists.hpp

// the 64 bits of a position image from position p on (one word of padding behind the last position: wi + 1 is always in range)
__device__ __forceinline__ uint64_t distinct_image_window(const uint64_t *bits, uint64_t p) {
    const uint64_t wi = p >> 6;
    const uint32_t sh = (uint32_t)(p & 63u);
    const uint64_t lo = bits[wi], hi = bits[wi + 1];
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

// ------------------------------------------------------------------------------------
// distinct_stream_kernel
//
// masked_stream_kernel's STREAM_TOPK pass, restated: its grid (row block, probe rank, query), its 4 independent waves per block,
// its walk over 64-position windows with the queue in a register and the compaction through the idle tile area, its chain
// arithmetic element for element, its keys (d2 bits << 32) | (u32)(cbase + position) and its statistics words.  A window's 64
// bits are the funnel-shifted words of the group column's validity image ANDed with those of the shared mask -- all ones where the
// call has neither -- clipped to the range and the cap exactly as there: a NULL-key row belongs to no group and is never read.
// What is new: lane l loads its row's group value key_pos[lbeg + my_r] (one gathered 4- / 8-byte load per evaluated row, issued
// ahead of the chain) and offers (key, storage row, group) to a WaveDistinctTopk.  The wave's list goes to part_keys / part_vals /
// part_grp [nq][n_part][k], group values widened to i64.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
__global__ __launch_bounds__(256) void distinct_stream_kernel(const StreamArgs a, const DistinctArgs da) {
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
            if (da.valid_pos) win &= distinct_image_window(da.valid_pos, p);
            if (da.bits) win &= distinct_image_window(da.bits, p);
            if (r1 - w0 < 64) win &= (1ull << (r1 - w0)) - 1ull;
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

#undef LDS_AT

template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
static hipError_t launch_distinct_t(const StreamArgs &a, const DistinctArgs &da, hipStream_t s) {
    dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
    hipLaunchKernelGGL((distinct_stream_kernel<CG, S, SEQ, ALIGNED, GW>), grid, dim3(256), 0, s, a, da);
    return hipGetLastError();
}

// the chunk choice of launch_stream (the chain order does not depend on it)
template <int S, int GW>
static hipError_t launch_distinct_s(const StreamArgs &a, const DistinctArgs &da, hipStream_t s) {
    const bool aligned = (a.dim % 4) == 0;
    const uint32_t G = a.dim / 4;
    if (a.metric == 1) {
        return aligned ? launch_distinct_t<16, S, true, true, GW>(a, da, s) : launch_distinct_t<16, S, true, false, GW>(a, da, s);
    }
    if (!aligned) return launch_distinct_t<32, S, false, false, GW>(a, da, s);
    if (G >= 64 && G % 64 == 0) return launch_distinct_t<64, S, false, true, GW>(a, da, s);
    return launch_distinct_t<32, S, false, true, GW>(a, da, s);
}

template <int GW>
static hipError_t launch_distinct_w(const StreamArgs &a, const DistinctArgs &da, hipStream_t s) {
    if (a.k <= 64) return launch_distinct_s<1, GW>(a, da, s);
    if (a.k <= 256) return launch_distinct_s<4, GW>(a, da, s);
    if (a.k <= 1024) return launch_distinct_s<16, GW>(a, da, s);
    return hipErrorInvalidValue;
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
    if (a.k <= 64) {
        if (w) hipLaunchKernelGGL((distinct_merge_kernel<1, 2>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((distinct_merge_kernel<1, 1>), grid, block, 0, s, a);
    } else if (a.k <= 256) {
        if (w) hipLaunchKernelGGL((distinct_merge_kernel<4, 2>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((distinct_merge_kernel<4, 1>), grid, block, 0, s, a);
    } else if (a.k <= 1024) {
        if (w) hipLaunchKernelGGL((distinct_merge_kernel<16, 2>), grid, block, 0, s, a);
        else hipLaunchKernelGGL((distinct_merge_kernel<16, 1>), grid, block, 0, s, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace pqv
