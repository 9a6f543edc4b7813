// half_tile.hpp -- the chain tile of 2-byte rows (chain_tile_h) and its loads, shared by every kernel that evaluates the reference
// chain on an f16 corpus: stream_h_kernel (kernels_half.hip), half_seed_kernel and survivor_h_kernel (kernels_half_screen.hip).
#ifndef PQV_HALF_TILE_HPP
#define PQV_HALF_TILE_HPP
#include "stream_walk.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// Eight halves of a row: one 16-byte load.  ALIGN = what the row starts are known to be aligned to -- 16 (dim % 8 == 0): one
// dwordx4; 4 (dim even): four dwords; 2: eight ushorts.  `full` = false: only the first four halves are the row's (the last
// half-load of a row whose dimension has an odd number of 4-groups) -- the other eight bytes may lie behind the corpus' last byte
// and are NOT read.
// ------------------------------------------------------------------------------------
struct Half8 { uint32_t w[4]; };

template <int ALIGN>
__device__ __forceinline__ Half8 load_h8(const uint16_t *p, bool full) {
    Half8 v;
    if constexpr (ALIGN == 16) {
        const uint4 t = *reinterpret_cast<const uint4 *>(p);
        v.w[0] = t.x; v.w[1] = t.y; v.w[2] = t.z; v.w[3] = t.w;
    } else if constexpr (ALIGN == 4) {
        const uint32_t *pw = reinterpret_cast<const uint32_t *>(p);
        v.w[0] = pw[0]; v.w[1] = pw[1];
        v.w[2] = full ? pw[2] : 0u; v.w[3] = full ? pw[3] : 0u;
    } else {
        v.w[0] = (uint32_t)p[0] | ((uint32_t)p[1] << 16); v.w[1] = (uint32_t)p[2] | ((uint32_t)p[3] << 16);
        v.w[2] = full ? (uint32_t)p[4] | ((uint32_t)p[5] << 16) : 0u; v.w[3] = full ? (uint32_t)p[6] | ((uint32_t)p[7] << 16) : 0u;
    }
    return v;
}
// binary16 bits -> f32 by the hardware conversion (v_cvt_f32_f16): exact for every half, subnormals included (the f16 denormal
// mode of a HIP kernel is IEEE; the units are not built with any flush-to-zero option)
__device__ __forceinline__ float widen_h(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16); }
__device__ __forceinline__ float4 widen_lo4(const Half8 &v) { return make_float4(widen_h(v.w[0] & 0xFFFFu), widen_h(v.w[0] >> 16), widen_h(v.w[1] & 0xFFFFu), widen_h(v.w[1] >> 16)); }
__device__ __forceinline__ float4 widen_hi4(const Half8 &v) { return make_float4(widen_h(v.w[2] & 0xFFFFu), widen_h(v.w[2] >> 16), widen_h(v.w[3] & 0xFFFFu), widen_h(v.w[3] >> 16)); }

// ------------------------------------------------------------------------------------
// The chain tile of 2-byte rows.  A chunk is CGH half-loads = 2 CGH of the reference's 4-groups of the dimension; a load
// instruction reads 64 x 16 B fully coalesced (CGH = 32: two 512-byte row segments = 256 dims each), NB = 8 of them in flight per
// lane.  A lane widens its eight halves and forms BOTH groups' partials t = ((d0^2 + d1^2) + d2^2) + d3^2 (SEQ: eight squares):
// chain elements 2h and 2h + 1 (SEQ: 8h .. 8h + 7) of its row.  The wave's tile is [slot][row] with chain_tile's XOR swizzle, and
// chain element e lives in slot (e % EPL) * CGH + e / EPL: the lanes of one store then write consecutive slots (no bank conflict,
// as with chain_tile's one partial per lane), and a chain read is one slot across 64 rows (conflict-free by the swizzle).  Lane r
// then replays row r's serial sum += t in ascending element order, and the dim % 4 tail element by element (index.rs:474-478).
// Budget: CGH 32 (SEQ: 8) -> 64 slots x 64 rows x 4 B = 16 KiB per wave, 64 KiB per block, chain_tile's CG = 64 budget.
// ------------------------------------------------------------------------------------
template <int CGH, bool SEQ>
constexpr int tile_words_h() { return CGH * (SEQ ? 8 : 2) * 64; }

template <int CGH, bool SEQ, int ALIGN>
__device__ __forceinline__ float chain_tile_h(const StreamArgs &a, float *lds, const float *qv, uint32_t my_srow, uint32_t nvalid, int lane) {
    constexpr int RPI = 64 / CGH;       // rows per load instruction
    constexpr int NI = CGH;             // load instructions per 64-row tile
    constexpr int EPL = SEQ ? 8 : 2;    // chain elements per lane item
    constexpr int NB = 8;               // loads in flight per lane
    constexpr bool QALIGNED = ALIGN == 16;      // (query rows are f32: 16-byte aligned where dim % 4 == 0; every full-load form has dim % 8 == 0)
    static_assert(NI % NB == 0, "NI must be a multiple of NB");
    const uint32_t dim = a.dim;
    const uint32_t G = dim >> 2;            // the reference's 4-groups
    const uint32_t H = (G + 1) >> 1;        // half-loads that cover them; the last one is HALF a load where G is odd
    const uint32_t tail = dim & 3u;
    const int h_in = lane % CGH;     // my half-load inside a chunk
    const int row_in = lane / CGH;   // my row inside a load instruction
    auto slot = [](uint32_t e) { return (e % EPL) * CGH + e / EPL; };

    float sum = 0.0f;
    for (uint32_t c0 = 0; c0 < H; c0 += CGH) {
        const uint32_t nh = (H - c0 < (uint32_t)CGH) ? (H - c0) : (uint32_t)CGH;
        const bool hvalid = (uint32_t)h_in < nh;
        const uint32_t h = c0 + (hvalid ? h_in : 0);
        const bool full = ALIGN == 16 || 2 * h + 1 < G;       // both 4-groups of the load are the row's
        const uint32_t hoff = h * 8;
        const float4 qa = load4<QALIGNED>(qv + hoff);
        float4 qb = make_float4(0.f, 0.f, 0.f, 0.f);
        if (full) qb = load4<QALIGNED>(qv + hoff + 4);

#pragma unroll 1
        for (int ib = 0; ib < NI; ib += NB) {
            Half8 x[NB];
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                uint32_t rr = (uint32_t)((ib + u) * RPI + row_in);
                if (rr >= nvalid) rr = nvalid - 1;
                const uint32_t srow = (uint32_t)__shfl((int)my_srow, (int)rr, 64);
                x[u] = load_h8<ALIGN>(a.mat_h + (uint64_t)srow * dim + hoff, full);
            }
#pragma unroll
            for (int u = 0; u < NB; ++u) {
                const int rr = (ib + u) * RPI + row_in;
                const float4 xa = widen_lo4(x[u]), xb = widen_hi4(x[u]);
                const float d0 = qa.x - xa.x, d1 = qa.y - xa.y, d2 = qa.z - xa.z, d3 = qa.w - xa.w;
                const float d4 = qb.x - xb.x, d5 = qb.y - xb.y, d6 = qb.z - xb.z, d7 = qb.w - xb.w;
                if constexpr (SEQ) {
                    if (hvalid) {
                        lds_at(lds, 0 * CGH + h_in, rr) = d0 * d0;
                        lds_at(lds, 1 * CGH + h_in, rr) = d1 * d1;
                        lds_at(lds, 2 * CGH + h_in, rr) = d2 * d2;
                        lds_at(lds, 3 * CGH + h_in, rr) = d3 * d3;
                        if (full) {
                            lds_at(lds, 4 * CGH + h_in, rr) = d4 * d4;
                            lds_at(lds, 5 * CGH + h_in, rr) = d5 * d5;
                            lds_at(lds, 6 * CGH + h_in, rr) = d6 * d6;
                            lds_at(lds, 7 * CGH + h_in, rr) = d7 * d7;
                        }
                    }
                } else {
                    float ta = d0 * d0 + d1 * d1;
                    ta = ta + d2 * d2;
                    ta = ta + d3 * d3;
                    float tb = d4 * d4 + d5 * d5;
                    tb = tb + d6 * d6;
                    tb = tb + d7 * d7;
                    if (hvalid) {
                        lds_at(lds, h_in, rr) = ta;
                        if (full) lds_at(lds, CGH + h_in, rr) = tb;
                    }
                }
            }
        }
        wave_lds_fence();
        // the chunk's chain elements: its 4-groups (the last half-load of an odd G holds one), SEQ: four squares each
        const uint32_t ng = (G - 2 * c0 < 2u * CGH) ? (G - 2 * c0) : 2u * CGH;
        const uint32_t nchain = ng * (SEQ ? 4u : 1u);
        uint32_t e = 0;
        for (; e + 8 <= nchain; e += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = lds_at(lds, slot(e + u), lane);
#pragma unroll
            for (int u = 0; u < 8; ++u) sum = sum + v[u];
        }
        for (; e < nchain; ++e) sum = sum + lds_at(lds, slot(e), lane);
        wave_lds_fence();
    }
    if (tail) {  // scalar tail of squared_l2_distance (index.rs:474-478)
        const uint16_t *xr = a.mat_h + (uint64_t)my_srow * dim + (uint64_t)G * 4;
        const float *qt = qv + (uint64_t)G * 4;
        for (uint32_t e = 0; e < tail; ++e) {
            const float d = qt[e] - widen_h(xr[e]);
            sum = sum + d * d;
        }
    }
    return sum;
}

}  // namespace pqv

#endif  // PQV_HALF_TILE_HPP
