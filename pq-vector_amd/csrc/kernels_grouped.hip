// kernels_grouped.hip -- gfx950 kernels of the grouped top-k (pqv.h: pqv_topk_grouped): up to group_size rows of each of the k
// nearest groups.  The call is two passes over the same candidates.  Pass 1 is the distinct call as it stands (kernels_distinct.hip)
// and names the k groups; everything here is pass 2, which knows a row's group before it reads the row:
//
//   group_set_kernel        the first n_found group values of a query, sorted ascending, each with its rank in pass 1 (its SLOT)
//   WaveGroupedTopk<S>      a wave-distributed list ascending by (slot, key) that holds at most group_size entries per slot
//   grouped_stream_kernel   distinct_stream_kernel's exact walk over the positions whose group value is in the query's set
//   grouped_merge_kernel    one wave per query folds the per-wave partial lists through the same offer and writes [q][slot][i]
//
// Why no one-pass list: with several rows per group a row refused because its group is not among the k nearest NOW may be the
// second best of a group that a later, nearer row pulls in, and a kept row of a near group can have any number of rows of other
// groups in front of it -- no bounded (d2, position) list is exact.  With the groups fixed, every slot is an independent
// "group_size smallest keys" selection, and the list below is k of those side by side.
//
// The invariant (tests/test_grouped_host.py models it): after any sequence of offers, slot g's entries are the min(group_size,
// offered) smallest keys offered for g.  An offer inserts while g holds fewer than group_size entries, else replaces g's largest
// entry if the candidate is smaller; neither touches another slot's set.  Only members of the k groups are offered, so the list
// holds at most k * group_size <= S * 64 entries: it cannot overflow and needs no admission threshold.
//
// The fold is exact for the plain reason: each of slot g's global group_size smallest keys is among the group_size smallest of
// the partition that holds it, so it reaches the fold, where the same offer keeps the smallest per slot.
#include "wave_group_lists.hpp"

namespace pqv {

// GROUPED_SLOT_EMPTY, WaveGroupedTopk<S>: wave_group_lists.hpp

// the 64 bits of a position image from position p on (distinct_image_window: one word of padding behind the last position)
__device__ __forceinline__ uint64_t grouped_image_window(const uint64_t *bits, uint64_t p) {
    const uint64_t wi = p >> 6;
    const uint32_t sh = (uint32_t)(p & 63u);
    const uint64_t lo = bits[wi], hi = bits[wi + 1];
    return sh ? (lo >> sh) | (hi << (64u - sh)) : lo;
}

// ------------------------------------------------------------------------------------
// group_set_kernel: one block per query.  Reads the first n_found[q] group values of pass 1 -- never the padding behind them, whose 0
// may be a real group -- and writes them ascending (rank counting in LDS: the values are distinct) with each value's slot, its
// rank in pass 1, to set_keys / set_slot [nq][k].  k <= GROUPED_SET_MAX.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_set_kernel(const int64_t *group_key, const uint32_t *n_found, uint32_t k, int64_t *set_keys,
                                                        uint32_t *set_slot) {
    __shared__ int64_t vals[GROUPED_SET_MAX];
    const uint32_t q = blockIdx.x;
    uint32_t n = n_found[q];
    if (n > k) n = k;
    const uint64_t base = (uint64_t)q * k;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) vals[i] = group_key[base + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int64_t v = vals[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += vals[j] < v ? 1u : 0u;
        set_keys[base + rank] = v;
        set_slot[base + rank] = i;
    }
}

hipError_t launch_group_set(const int64_t *group_key, const uint32_t *n_found, uint32_t nq, uint32_t k, int64_t *set_keys, uint32_t *set_slot,
                            hipStream_t s) {
    if (!group_key || !n_found || !set_keys || !set_slot || k == 0 || k > GROUPED_SET_MAX) return hipErrorInvalidValue;
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(group_set_kernel, dim3(nq), dim3(256), 0, s, group_key, n_found, k, set_keys, set_slot);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// grouped_stream_kernel
//
// distinct_stream_kernel's walk, restated: its grid (row block, probe rank, query), its 4 independent waves per block, its cap /
// pair_end / max_pos clamp, its walk over 64-position windows with the queue in a register and the compaction through the idle tile
// area, its chain arithmetic element for element -- so a row's d2 has the bits pass 1 gave it -- and its keys.  A window's 64 bits
// are the AND of three sources: the group column's validity image, the shared mask's image, and MEMBERSHIP -- lane l reads
// key_pos[p + l] (one coalesced window, as the keyed kernel reads it), sign-extends an i32 value, and looks it up in the query's
// sorted set by a branch-free binary search over full i64 values.  The set (5 KB: GROUPED_SET_MAX i64 values and u16 slots) is
// staged once per block in LDS beside the tile area.  A row outside the k groups is never read.  The slot found by the lookup
// travels through the queue beside the list offset, and lane l offers (key, storage row, slot) to a WaveGroupedTopk.
//
// The wave writes the filled part of its list to part_keys / part_vals / part_slot [nq][n_part][km] and the length to part_cnt
// [nq][n_part]: most waves of a call meet a handful of members, and the fold reads what was written, not km entries per wave.
// Statistics: the rows evaluated here are added to the embeddings_fetched word; candidate_rows was counted by pass 1.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
__global__ __launch_bounds__(256) void grouped_stream_kernel(const StreamArgs a, const GroupedArgs ga) {
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
    // the query's set (block-uniform; every wave of the block passes the barrier before it looks at its range)
    uint32_t set_n = ga.n_found[q];
    if (set_n > ga.k) set_n = ga.k;
    for (uint32_t i = threadIdx.x; i < set_n; i += 256) {
        set_v[i] = ga.set_keys[(uint64_t)q * ga.k + i];
        set_s[i] = (uint16_t)ga.set_slot[(uint64_t)q * ga.k + i];
    }
    __syncthreads();

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
            if (ga.valid_pos) win &= grouped_image_window(ga.valid_pos, p);
            if (ga.bits) win &= grouped_image_window(ga.bits, p);
            if (r1 - w0 < 64) win &= (1ull << (r1 - w0)) - 1ull;
            if (win == 0) continue;
            // membership: my position's group value (p + lane < the image's n_words * 64) against the sorted set
            int64_t kv;
            if constexpr (GW == 1) kv = (int64_t) static_cast<const int32_t *>(ga.key_pos)[p + (uint64_t)lane];
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

template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
static hipError_t launch_grouped_t(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
    hipLaunchKernelGGL((grouped_stream_kernel<CG, S, SEQ, ALIGNED, GW>), grid, dim3(256), 0, s, a, ga);
    return hipGetLastError();
}

// the chunk choice of launch_stream (the chain order does not depend on it)
template <int S, int GW>
static hipError_t launch_grouped_s(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    const bool aligned = (a.dim % 4) == 0;
    const uint32_t G = a.dim / 4;
    if (a.metric == 1) {
        return aligned ? launch_grouped_t<16, S, true, true, GW>(a, ga, s) : launch_grouped_t<16, S, true, false, GW>(a, ga, s);
    }
    if (!aligned) return launch_grouped_t<32, S, false, false, GW>(a, ga, s);
    if (G >= 64 && G % 64 == 0) return launch_grouped_t<64, S, false, true, GW>(a, ga, s);
    return launch_grouped_t<32, S, false, true, GW>(a, ga, s);
}

template <int GW>
static hipError_t launch_grouped_w(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    if (ga.km <= 64) return launch_grouped_s<1, GW>(a, ga, s);
    if (ga.km <= 256) return launch_grouped_s<4, GW>(a, ga, s);
    return launch_grouped_s<16, GW>(a, ga, s);
}

// k * group_size <= 1024 with group_size >= 2 (one row per group is the distinct call), hence k <= GROUPED_SET_MAX
static bool grouped_shape_ok(uint32_t k, uint32_t group_size, uint32_t km) {
    return k != 0 && group_size >= 2 && (uint64_t)k * group_size == km && km <= 1024 && k <= GROUPED_SET_MAX;
}

hipError_t launch_grouped_stream(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base || !ga.part_keys || !ga.part_vals || !ga.part_slot || !ga.part_cnt) return hipErrorInvalidValue;
    if (!ga.key_pos || !ga.set_keys || !ga.set_slot || !ga.n_found || !grouped_shape_ok(ga.k, ga.group_size, ga.km)) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0 || a.nprobe == 0) return hipSuccess;
    if (ga.elem_size == 4) return launch_grouped_w<1>(a, ga, s);
    if (ga.elem_size == 8) return launch_grouped_w<2>(a, ga, s);
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------
// grouped_merge_kernel: one wave per query folds the query's n_part partial lists through WaveGroupedTopk::offer -- the lengths
// of 64 lists per load, then 64 entries of a list per step, only the filled ones.  The folded list is ascending by (slot, key), so
// the write-out is a segmented index: the list goes to LDS, the first entry of a segment records the segment's start and the
// last one its length, and output (g, i) is entry start[g] + i where i < rows[g], else the padding (0xFFFFFFFF, +inf).  Storage
// row -> reported row through ids, sqrt (IEEE) or the cosine halving as the distinct fold applies them.  group_rows[q][g] = rows[g]
// (0 for a slot with no group).  group_key and n_found are pass 1's.
// ------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void grouped_merge_kernel(const GroupedMergeArgs a) {
    __shared__ uint64_t l_key[S * 64];
    __shared__ uint32_t l_val[S * 64];
    __shared__ uint32_t l_start[GROUPED_SET_MAX];
    __shared__ uint32_t l_rows[GROUPED_SET_MAX];
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint32_t k = a.k, m = a.group_size, km = a.km;
    WaveGroupedTopk<S> tk;
    tk.init();

    for (uint32_t p0 = 0; p0 < a.n_part; p0 += 64) {
        const uint32_t pl = p0 + (uint32_t)lane;
        uint32_t mycnt = pl < a.n_part ? a.part_cnt[(uint64_t)q * a.n_part + pl] : 0u;
        if (mycnt > km) mycnt = km;
        unsigned long long todo = __ballot(mycnt != 0);
        while (todo) {
            const int L = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t cnt = readlane_u32(mycnt, L);
            const uint64_t base = ((uint64_t)q * a.n_part + p0 + (uint32_t)L) * km;
            for (uint32_t e0 = 0; e0 < cnt; e0 += 64) {
                const uint32_t e = e0 + (uint32_t)lane;
                const bool in = e < cnt;
                const uint64_t kv = in ? a.part_keys[base + e] : KEY_EMPTY;
                const uint32_t vv = in ? a.part_vals[base + e] : 0xFFFFFFFFu;
                const uint32_t sv = in ? a.part_slot[base + e] : 0u;
                // (a slot at or beyond k cannot come from the stream kernel; kept out so that no index below leaves its array)
                tk.offer(in && sv < k ? kv : KEY_EMPTY, vv, sv, m, lane);
            }
        }
    }

    for (uint32_t g = lane; g < k; g += 64) l_rows[g] = 0;
    wave_lds_fence();
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        l_key[e] = tk.key[s];
        l_val[e] = tk.val[s];
        // the slot of element e - 1 (lane 0: the last lane of the register below; element 0: none)
        uint32_t prev = (uint32_t)__shfl_up((int)tk.slot[s], 1, 64);
        const uint32_t below = s > 0 ? readlane_u32(tk.slot[s > 0 ? s - 1 : 0], 63) : GROUPED_SLOT_EMPTY;
        if (lane == 0) prev = below;
        const uint32_t mine = tk.slot[s];
        if (e < tk.n && prev != mine) l_start[mine] = e;
    }
    wave_lds_fence();
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        // the slot of element e + 1 (lane 63: the first lane of the register above; the last element: none)
        uint32_t next = (uint32_t)__shfl_down((int)tk.slot[s], 1, 64);
        const uint32_t above = s + 1 < S ? readlane_u32(tk.slot[s + 1 < S ? s + 1 : s], 0) : GROUPED_SLOT_EMPTY;
        if (lane == 63) next = above;
        const uint32_t mine = tk.slot[s];
        if (e < tk.n && next != mine) l_rows[mine] = e + 1 - l_start[mine];
    }
    wave_lds_fence();

    const uint64_t obase = (uint64_t)q * km;
    for (uint32_t o = lane; o < km; o += 64) {
        const uint32_t g = o / m, i = o - g * m;
        uint32_t row = 0xFFFFFFFFu;
        float d = INFINITY;
        if (i < l_rows[g]) {
            const uint32_t e = l_start[g] + i;
            const float d2 = __uint_as_float((uint32_t)(l_key[e] >> 32));
            row = a.ids ? a.ids[l_val[e]] : l_val[e];
            d = a.sqrt_out == 1 ? sqrt_f32_ieee(d2) : a.sqrt_out == 2 ? 0.5f * d2 : d2;
        }
        a.row_idx[obase + o] = row;
        a.dist[obase + o] = d;
    }
    if (a.group_rows)
        for (uint32_t g = lane; g < k; g += 64) a.group_rows[(uint64_t)q * k + g] = l_rows[g];
}

hipError_t launch_grouped_merge(const GroupedMergeArgs &a, hipStream_t s) {
    if (!a.part_keys || !a.part_vals || !a.part_slot || !a.part_cnt || !a.row_idx || !a.dist) return hipErrorInvalidValue;
    if (!grouped_shape_ok(a.k, a.group_size, a.km)) return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    const dim3 grid(a.nq), block(64);
    if (a.km <= 64) hipLaunchKernelGGL((grouped_merge_kernel<1>), grid, block, 0, s, a);
    else if (a.km <= 256) hipLaunchKernelGGL((grouped_merge_kernel<4>), grid, block, 0, s, a);
    else hipLaunchKernelGGL((grouped_merge_kernel<16>), grid, block, 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// group_rows_fill_kernel: group_size == 1 takes the distinct call as it stands, whose groups have one row each:
// group_rows[q][g] = g < n_found[q].
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_rows_fill_kernel(const uint32_t *n_found, uint32_t nq, uint32_t k, uint32_t *group_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * k) return;
    group_rows[i] = (uint32_t)(i % k) < n_found[i / k] ? 1u : 0u;
}

hipError_t launch_group_rows_fill(const uint32_t *n_found, uint32_t nq, uint32_t k, uint32_t *group_rows, hipStream_t s) {
    if (!n_found || !group_rows || k == 0) return hipErrorInvalidValue;
    if (nq == 0) return hipSuccess;
    const uint64_t n = (uint64_t)nq * k;
    hipLaunchKernelGGL(group_rows_fill_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, n_found, nq, k, group_rows);
    return hipGetLastError();
}

}  // namespace pqv
