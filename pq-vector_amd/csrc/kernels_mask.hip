// kernels_mask.hip -- gfx950 kernels of the row-masked searches (pqv.h: pqv_row_mask): mask_layout_kernel (allow bytes in row
// order -> a bitset indexed by LIST POSITION) and masked_stream_kernel (stream_kernel's exact distance pass over the allowed
// positions only) -- and of the per-query key filters (pqv.h: pqv_row_keys): key_layout_kernel (a key column in row order -> list
// position order) and masked_stream_kernel's keyed instantiations, whose windows come from comparing keys.  The screened paths take their thresholds from sampled rows; a threshold from a row the mask excludes is no
// bound on the masked answer, so masked calls always run this exact pass.
#include "device_common.hpp"

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
// stream_kernel's grid (row block, probe rank, query), its 4 independent waves per block and its chain arithmetic, element for
// element (REF4 groups / SEQ squares, dim % 4 tails, unaligned rows; the unit is built with -ffp-contract=off like the others).
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

template <int CG, int S, int MODE, bool SEQ, bool ALIGNED, int WIN = 0>
__global__ __launch_bounds__(256) void masked_stream_kernel(const StreamArgs a, const typename WinArgs<WIN>::type ma) {
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

    const uint32_t q = blockIdx.z, j = blockIdx.y + (MODE == STREAM_RANGE ? a.j0 : 0u);
    if constexpr (MODE == STREAM_TOPK) {
        // a rank at or beyond the query's limit (pqv_topk_expand) walks nothing: that one word is all the block loads, its four
        // waves' lists go out EMPTY for the final merge (block-uniform: nobody is left waiting at the IN forms' barrier)
        if (ma.rank_limit && j >= ma.rank_limit[q]) {
            const uint32_t n_part = a.nprobe * a.blocks_per_list * 4;
            const uint64_t base = ((uint64_t)q * n_part + (j * a.blocks_per_list + blockIdx.x) * 4 + wave) * a.k;
            for (uint32_t e = lane; e < a.k; e += 64) {
                a.part_keys[base + e] = KEY_EMPTY;
                a.part_vals[base + e] = 0xFFFFFFFFu;
            }
            return;
        }
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

#ifdef PQV_PROFILE_PHASES
    unsigned long long *st = ma.stats;
#else
    unsigned long long *st = ma.stats ? ma.stats + 8 + 16 * (q % STATS_SLOTS) : nullptr;
#endif
    if (ma.n_cand && st && blockIdx.x == 0 && j == 0 && threadIdx.x == 0) atomicAdd(&st[2], (unsigned long long)ma.n_cand[q]);

    int64_t qkey = 0;
    if constexpr (WIN == 1 || WIN == 2) qkey = ma.qkeys[q];
    int64_t qhi = 0;            // WIN 3 / 4: the window is qkey <= kv && kv <= qhi
    if constexpr (WIN == 3 || WIN == 4) {
        qkey = static_cast<const int64_t *>(ma.a)[q];
        qhi = static_cast<const int64_t *>(ma.b)[q];
    }
    const int64_t *kset = nullptr;
    uint32_t kset_n = 0;        // WIN 5 / 6: the values of the query's set held in kset (block-uniform)
    if constexpr (WIN >= 5) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        const uint64_t s0 = static_cast<const uint64_t *>(ma.a)[q], s1 = static_cast<const uint64_t *>(ma.a)[q + 1];
        if (s1 > s0) kset_n = s1 - s0 > (uint64_t)KEY_SET_MAX ? KEY_SET_MAX : (uint32_t)(s1 - s0);
        for (uint32_t i = threadIdx.x; i < kset_n; i += 256) set_lds[i] = static_cast<const int64_t *>(ma.b)[s0 + i];
        __syncthreads();
        kset = set_lds;
        if (kset_n == 0) r1 = r0;      // (nothing matches: no window is read)
    }

    const uint32_t dim = a.dim;
    const uint32_t G = dim >> 2;
    const uint32_t tail = dim & 3u;
    const float *qv = a.queries + (uint64_t)q * dim;
    const int g_in = lane % CG;      // my float4 group inside a chunk
    const int row_in = lane / CG;    // my row inside a load instruction

    WaveTopk<S> tk;
    if constexpr (MODE == STREAM_TOPK) tk.init();

    uint32_t pend = 0;      // queue entry `lane` (a list offset, < 2^32 as every candidate position), meaningful for lane < qn
    uint32_t qn = 0;        // queued entries, < 64 between two windows (wave-uniform)
    uint32_t n_eval = 0;    // rows this wave evaluated (wave-uniform)
    for (uint64_t w0 = r0;; w0 += 64) {
        const bool flush = w0 >= r1;        // past the range: what is left in the queue is the last tile
        uint32_t nvalid = 0;                // rows of the chain tile this turn runs (0: none)
        uint32_t my_r = 0;                  // list offset of tile row `lane`
        if (!flush) {
            const uint64_t p = lbeg + w0;
            uint64_t win;
            if constexpr (WIN == 0) {
                win = image_window(ma.bits, p);
            } else {
                // (key_pos is padded by a whole window: p + lane is always in range; positions >= r1 are clipped below)
                int64_t kv;
                if constexpr (WIN & 1) kv = (int64_t) static_cast<const int32_t *>(ma.key_pos)[p + (uint64_t)lane];
                else kv = static_cast<const int64_t *>(ma.key_pos)[p + (uint64_t)lane];
                if constexpr (WIN <= 2) {
                    win = __ballot(kv == qkey);
                } else if constexpr (WIN <= 4) {
                    win = __ballot(qkey <= kv && kv <= qhi);
                } else {
                    uint32_t at = 0;
                    for (uint32_t span = kset_n; span > 1;) {           // (wave-uniform trip count; at + half < kset_n)
                        const uint32_t half = span >> 1;
                        if (kset[at + half] <= kv) at += half;
                        span -= half;
                    }
                    win = __ballot(kset[at] == kv);                     // (kset_n >= 1 here)
                }
                if (ma.valid_pos) win &= image_window(ma.valid_pos, p);
                if (ma.bits) win &= image_window(ma.bits, p);
            }
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
            if (tail) {  // scalar tail of squared_l2_distance (index.rs:474-478)
                const float *xr = a.mat + (uint64_t)my_srow * dim + (uint64_t)G * 4;
                const float *qt = qv + (uint64_t)G * 4;
                for (uint32_t e = 0; e < tail; ++e) {
                    const float d = qt[e] - xr[e];
                    sum = sum + d * d;
                }
            }

            const uint64_t pos = cbase + my_r;
            const bool valid = (uint32_t)lane < nvalid;           // (pos < lim by the clamp of the walk)
            if constexpr (MODE == STREAM_TOPK) {
                const uint64_t mykey =
                    valid ? (((uint64_t)__float_as_uint(sum) << 32) | (uint64_t)(uint32_t)pos)
                          : KEY_EMPTY;
                tk.offer(mykey, my_srow, a.k, lane);
            } else {
                // the wave's hits go to the query's segment in one block: ballot, rank from mbcnt, one atomicAdd per wave
                const float outv = a.sqrt_out == 1 ? sqrt_f32_ieee(sum) : a.sqrt_out == 2 ? 0.5f * sum : sum;     // (2: PQV_COSINE)
                const bool hit = valid && outv <= a.radius;                // (a NaN distance never compares true)
                const uint64_t m = __ballot(hit);
                if (m) {
                    uint32_t base = 0;
                    if (lane == 0) base = atomicAdd(a.hit_cnt + q, (uint32_t)__popcll(m));
                    base = (uint32_t)__shfl((int)base, 0, 64);
                    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
                    if (hit) {
                        const uint64_t o = (uint64_t)q * a.seg_stride + base + rank;
                        a.hit_keys[o] = ((uint64_t)__float_as_uint(sum) << 32) | (uint64_t)(uint32_t)pos;
                        a.hit_vals[o] = my_srow;
                    }
                }
            }
        }
        if (flush) break;
    }
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    if constexpr (MODE == STREAM_TOPK) {
        const uint32_t n_part = a.nprobe * a.blocks_per_list * 4;
        const uint32_t pi = (j * a.blocks_per_list + blockIdx.x) * 4 + wave;
        const uint64_t base = ((uint64_t)q * n_part + pi) * a.k;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            const uint32_t e = s * 64 + lane;
            if (e < a.k) {
                a.part_keys[base + e] = tk.key[s];
                a.part_vals[base + e] = tk.val[s];
            }
        }
    }
}

#undef LDS_AT

template <int CG, int S, int MODE, bool SEQ, bool ALIGNED, int WIN>
static hipError_t launch_masked_t(const StreamArgs &a, const typename WinArgs<WIN>::type &ma, hipStream_t s) {
    dim3 grid(a.blocks_per_list, MODE == STREAM_RANGE ? a.nj : a.nprobe, a.nq);
    hipLaunchKernelGGL((masked_stream_kernel<CG, S, MODE, SEQ, ALIGNED, WIN>), grid, dim3(256), 0, s, a, ma);
    return hipGetLastError();
}

// the chunk choice of launch_stream (the chain order does not depend on it)
template <int S, int MODE, int WIN>
static hipError_t launch_masked_s(const StreamArgs &a, const typename WinArgs<WIN>::type &ma, hipStream_t s) {
    const bool aligned = (a.dim % 4) == 0;
    const uint32_t G = a.dim / 4;
    if (a.metric == 1) {
        return aligned ? launch_masked_t<16, S, MODE, true, true, WIN>(a, ma, s)
                       : launch_masked_t<16, S, MODE, true, false, WIN>(a, ma, s);
    }
    if (!aligned) return launch_masked_t<32, S, MODE, false, false, WIN>(a, ma, s);
    if (G >= 64 && G % 64 == 0) return launch_masked_t<64, S, MODE, false, true, WIN>(a, ma, s);
    return launch_masked_t<32, S, MODE, false, true, WIN>(a, ma, s);
}

template <int WIN>
static hipError_t launch_masked_w(const StreamArgs &a, const typename WinArgs<WIN>::type &ma, StreamMode mode, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0) return hipSuccess;
    if (mode == STREAM_RANGE) return a.nj == 0 ? hipSuccess : launch_masked_s<1, STREAM_RANGE, WIN>(a, ma, s);
    if (mode != STREAM_TOPK) return hipErrorInvalidValue;
    if (a.nprobe == 0) return hipSuccess;
    if (a.k <= 64) return launch_masked_s<1, STREAM_TOPK, WIN>(a, ma, s);
    if (a.k <= 256) return launch_masked_s<4, STREAM_TOPK, WIN>(a, ma, s);
    if (a.k <= 1024) return launch_masked_s<16, STREAM_TOPK, WIN>(a, ma, s);
    return hipErrorInvalidValue;
}

hipError_t launch_masked_stream(const StreamArgs &a, const MaskedArgs &ma, StreamMode mode, hipStream_t s) {
    if (!ma.bits) return hipErrorInvalidValue;
    return launch_masked_w<0>(a, ma, mode, s);
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
