// kernels_mmr.hip -- the gfx950 kernel of the MMR calls (pqv.h: pqv_mmr_select, pqv_topk_mmr): greedy maximal-marginal-relevance
// selection of k out of n <= 1024 candidates per query, the pairwise distances taken on the resident rows by the chain every
// search uses (chain_tile, stream_walk.hpp) with a picked ROW in the query's place.
//   mmr_select_kernel   one block per query; a candidate's state lives in the registers of the lane that owns its position
// Nothing is probed and nothing is screened: a candidate that is not considered -- its row in no list, or its position at or
// beyond the query's n_found_in -- is never loaded and never picked.
#include "stream_walk.hpp"

namespace pqv {

constexpr uint32_t MMR_NO_POS = 0xFFFFFFFFu;    // the row map's word for a row no list holds
constexpr int MMR_SLOTS = 4;                    // tiles per wave: 4 waves x 4 tiles x 64 lanes = the 1024 candidates a call takes

// element s of a lane's four (s wave-uniform or not): selects, so that the four stay in registers
template <class T>
__device__ __forceinline__ T pick4(const T (&v)[MMR_SLOTS], uint32_t s) { return s == 0 ? v[0] : s == 1 ? v[1] : s == 2 ? v[2] : v[3]; }
template <class T>
__device__ __forceinline__ void set4(T (&v)[MMR_SLOTS], uint32_t s, T x) {
#pragma unroll
    for (int u = 0; u < MMR_SLOTS; ++u) v[u] = s == (uint32_t)u ? x : v[u];
}
// the minimum of a 64-bit key across the wave, in every lane
__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
#pragma unroll
    for (int off = 32; off; off >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, off, 64);
        const uint32_t hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), off, 64);
        const uint64_t o = ((uint64_t)hi << 32) | (uint64_t)lo;
        v = o < v ? o : v;
    }
    return v;
}

// blocks of four waves a CU holds beside each other (a wave per SIMD each): what 160 KiB of LDS leave room for, at most 4
template <int CG, bool SEQ>
constexpr int mmr_blocks_per_cu() { return tile_words<CG, SEQ>() * 16 > 40 * 1024 ? 2 : 4; }

// ------------------------------------------------------------------------------------
// mmr_select_kernel
//
// grid = nq; block = 256 threads = 4 waves.  Wave w owns the 64-candidate tiles w, w + 4, w + 8, w + 12 of its query's n candidates
// (slot s = tile / 4), lane l of tile T the candidate at position T * 64 + l: its row id, its storage row (row map, then
// storage_row), rel, the running redundancy red and a live bit (considered and not yet picked) stay in registers.
// A step: every lane scores its live candidates -- (lambda * rel) - (om * red), three rounded f32 operations; red reads +0.0f
// while nothing is picked -- and the 64-bit keys (ord(score) << 32 | position) are reduced to their minimum across the wave, then
// across the four waves through three words per wave {key lo, key hi, the wave winner's storage row} at the head of each wave's tile
// area, between two block barriers: the area is idle between two chain tiles, and the second barrier keeps a wave's next tile from
// overwriting words another wave has not read yet.  The lane that owns the winning position writes the pick (row, rel bit for bit,
// the score from the key: ord is a bijection) and clears its live bit.  Unless that was the last pick, every wave then runs
// chain_tile over each of its tiles that still holds a live candidate, the winner's storage row in global memory as qv, and folds
// pd on the output scale into red where it is smaller (a NaN never is).  A tile's rows end at its last considered lane; a lane in
// between that is not considered follows the tile's first considered row, so every address chain_tile forms is a considered row's.
// The block ends when no live candidate is left (all keys KEY_EMPTY -- a real key's position is below 1024) or after k picks, pads
// the outputs behind the picks with 0xFFFFFFFF / +inf / +inf and writes n_found.
// Every access stays in bounds whatever cand_rows holds: a row id indexes the map only behind the compare against its length, and
// only a map word that is a list position reaches storage_row.
// ------------------------------------------------------------------------------------
template <int CG, bool SEQ, bool ALIGNED, bool DOT>
__global__ __launch_bounds__(256, (mmr_blocks_per_cu<CG, SEQ>())) void mmr_select_kernel(const StreamArgs a, const MmrArgs ma) {
    static_assert(tile_words<CG, SEQ>() >= 4, "the exchange needs three words of every wave's tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();
    uint32_t *xw = reinterpret_cast<uint32_t *>(lds);

    const uint32_t q = blockIdx.x;
    const uint64_t base = (uint64_t)q * ma.n;
    const uint64_t obase = (uint64_t)q * ma.k;
    uint32_t lim = ma.n;
    if (ma.n_found_in) {
        const uint32_t nf = uniform_word(ma.n_found_in + q);
        if (nf < lim) lim = nf;
    }

    uint32_t srow[MMR_SLOTS], row[MMR_SLOTS], tile_n[MMR_SLOTS];
    float rel[MMR_SLOTS], red[MMR_SLOTS];
    uint32_t live = 0;
#pragma unroll
    for (int s = 0; s < MMR_SLOTS; ++s) {
        const uint32_t pos = (uint32_t)((wave + 4 * s) * 64 + lane);
        uint32_t r = 0xFFFFFFFFu, lpos = MMR_NO_POS;
        float d = 0.0f;
        if (pos < lim) {
            r = ma.cand_rows[base + pos];
            d = ma.cand_dist[base + pos];
            if (r < ma.map_len) lpos = ma.map[r];
        }
        const bool on = lpos != MMR_NO_POS;
        const uint64_t m = __ballot(on);
        const uint32_t sr = on ? storage_row(a, lpos) : 0u;
        const uint32_t fill = (uint32_t)__shfl((int)sr, m ? __builtin_ctzll(m) : 0, 64);
        srow[s] = on ? sr : fill;
        tile_n[s] = m ? 64u - (uint32_t)__builtin_clzll(m) : 0u;
        row[s] = r; rel[s] = d; red[s] = 0.0f;
        if (on) live |= 1u << s;
    }

    const float lambda = ma.lambda;
    const float om = 1.0f - lambda;
    uint32_t picks = 0;
    while (picks < ma.k) {
        uint64_t best = KEY_EMPTY;
#pragma unroll
        for (int s = 0; s < MMR_SLOTS; ++s) {
            const float sc = (lambda * rel[s]) - (om * red[s]);
            const uint64_t key = ((uint64_t)dot_ord(sc) << 32) | (uint64_t)(uint32_t)((wave + 4 * s) * 64 + lane);
            if (((live >> s) & 1u) && key < best) best = key;
        }
        best = wave_min_u64(best);
        const uint32_t bp = (uint32_t)best;
        const uint32_t bs = (uint32_t)__shfl((int)pick4(srow, (bp >> 8) & 3u), (int)(bp & 63u), 64);
        if (lane == 0) { xw[0] = (uint32_t)best; xw[1] = (uint32_t)(best >> 32); xw[2] = bs; }
        __syncthreads();
        uint64_t win = KEY_EMPTY;
        uint32_t win_srow = 0;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const uint32_t *p = reinterpret_cast<const uint32_t *>(lds_all + w * tile_words<CG, SEQ>());
            const uint64_t key = ((uint64_t)p[1] << 32) | (uint64_t)p[0];
            const uint32_t sr = p[2];
            if (key < win) { win = key; win_srow = sr; }
        }
        __syncthreads();
        if (win == KEY_EMPTY) break;

        const uint32_t wp = (uint32_t)win;
        if (((wp >> 6) & 3u) == (uint32_t)wave && (wp & 63u) == (uint32_t)lane) {
            const uint32_t s = wp >> 8;
            ma.row_idx[obase + picks] = pick4(row, s);
            ma.dist[obase + picks] = pick4(rel, s);
            if (ma.score) ma.score[obase + picks] = dot_unord((uint32_t)(win >> 32));
            live &= ~(1u << s);
        }
        const bool first = picks == 0;
        ++picks;
        if (picks == ma.k) break;       // the last pick: no redundancy pass behind it

        const float *qv = a.mat + (uint64_t)win_srow * a.dim;
#pragma unroll 1
        for (uint32_t s = 0; s < (uint32_t)MMR_SLOTS; ++s) {
            const uint32_t nv = (uint32_t)__builtin_amdgcn_readfirstlane((int)pick4(tile_n, s));
            if (nv == 0 || __ballot((live >> s) & 1u) == 0) continue;
            const float sum = chain_tile<CG, SEQ, ALIGNED, DOT>(a, lds, qv, pick4(srow, s), nv, lane);
            float pd;
            if constexpr (DOT) pd = 0.0f - sum;
            else pd = a.sqrt_out == 1 ? sqrt_f32_ieee(sum) : a.sqrt_out == 2 ? 0.5f * sum : sum;
            const float r0 = first ? INFINITY : pick4(red, s);
            set4(red, s, pd < r0 ? pd : r0);
        }
    }

    for (uint32_t j = picks + threadIdx.x; j < ma.k; j += 256) {
        ma.row_idx[obase + j] = 0xFFFFFFFFu;
        ma.dist[obase + j] = INFINITY;
        if (ma.score) ma.score[obase + j] = INFINITY;
    }
    if (threadIdx.x == 0 && ma.n_found) ma.n_found[q] = picks;
}

hipError_t launch_mmr_select(const StreamArgs &a, const MmrArgs &ma, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (ma.n > 64u * 4u * MMR_SLOTS || ma.k == 0 || a.nq > 0x7FFFFFFFu) return hipErrorInvalidValue;
    if (!a.mat || !ma.row_idx || !ma.dist || (ma.n && (!ma.cand_rows || !ma.cand_dist))) return hipErrorInvalidValue;
    if ((ma.map_len && !ma.map) || ma.map_len > 0xFFFFFFFFull) return hipErrorInvalidValue;
    auto go = [&](auto dot) {
        return dispatch_chunk<!decltype(dot)::value>(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
            hipLaunchKernelGGL((mmr_select_kernel<cg.value, seq.value, aligned.value, decltype(dot)::value>), dim3(a.nq), dim3(256), 0, s, a, ma);
            return hipGetLastError();
        });
    };
    return a.metric == 4 ? go(std::true_type{}) : go(std::false_type{});      // PQV_DOT
}

}  // namespace pqv
