// kernels_build.hip -- index build (src/ivf/index.rs:323-457, :189-206): assign_f16_kernel + assign_rescore(_wave)_kernel (the k-means
// assignment as an f16 contraction + exact re-scoring), assign_kernel (exact VALU form), lloyd_update_kernel, and the helpers of
// the f32-screened assignment.
#include "device_common.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// Round 3: the k-means assignment (index.rs:395-430 Lloyd, :189-206 + :244-257 final) as a dense contraction on the f16
// matrix pipe + exact re-scoring -- the brute-force design with the roles swapped: every ROW keeps a threshold and a
// candidate list, the CENTROIDS are the streamed side.
//
//   images      x^ = (x - mu) / |x - mu| * 2^8 in f16 for rows and centroids alike (mu: any fixed vector -- the distance is
//               translation invariant; centring shrinks |x - mu| |c - mu| and with it the bound's slack)
//   assign_f16_kernel   one block = 128 rows against ALL centroids, 256 at a time (4 waves as 2 x 2, 64 rows x 128
//               centroids each, v_mfma_f32_32x32x16_f16, K in 32-value stages through double-buffered LDS).  With s~ the image
//               dot product / 2^16:  d~ = |a|^2 + |b|^2 - 2 |a||b| s~,  |d~ - d| <= err = 2 |a||b| eps + 4e-6 (|a|^2 + |b|^2)
//               (eps as in brute_f16_kernel), and the reference's computed distance lies within (1 +- cm) of d.  Per row the
//               smallest UPPER bound seen so far is a running threshold (LDS); every centroid whose LOWER bound does not
//               exceed it is appended to the row's candidate list.  The true argmin is never dropped: its lower bound is
//               below its own upper bound, which is below every threshold the row ever had.
//   assign_rescore_kernel   exact reference-order distances (index.rs:461-480) of a row's candidates, four lanes per row,
//               argmin by (distance bits, centroid index) = strict '<' in ascending index order; a row whose list
//               overflowed is compared with every centroid.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void assign_f16_kernel(const AssignF16Args a) {
    __shared__ float4 As4[2][BH_BM * 4];
    __shared__ float4 Bs4[2][BH_BN * 4];
    __shared__ uint32_t thr_s[BH_BM];        // running threshold per row: bits of a non-negative float
    __shared__ float xn2_s[BH_BM];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const uint64_t m0 = (uint64_t)blockIdx.x * BH_BM;
    const uint32_t dp = a.dim_p;
    const int ld_r = tid >> 2, ld_ch = tid & 3;
    float4 ra[2], rb[4];
    const uint64_t qleft = (a.m - m0) * dp * 2;
    const __amdgpu_buffer_rsrc_t qres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t *>(a.x16 + m0 * dp), 0, (int)(qleft > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)qleft), 0x00020000);
    const uint32_t lane_b = (uint32_t)ld_r * dp * 2 + (uint32_t)ld_ch * 16, r64_b = 64u * dp * 2;
    __shared__ float xs_s[BH_BM];            // |row - mu| (the square roots are taken once per row / centroid, not per pair)
    if (tid < BH_BM) {
        thr_s[tid] = 0x7F800000u;            // +inf
        const float xn = m0 + tid < a.m ? a.xn2[m0 + tid] : 0.0f;
        xn2_s[tid] = xn;
        xs_s[tid] = sqrtf(xn) * 1.000001f;
    }
    const int l31 = lane & 31, lk = lane >> 5;
    int rowa[2], rowb[4], swa[2], swb[4];
#pragma unroll
    for (int t = 0; t < 2; ++t) { rowa[t] = wm * 64 + t * 32 + l31; swa[t] = (rowa[t] >> 2) & 3; }
#pragma unroll
    for (int t = 0; t < 4; ++t) { rowb[t] = wn * 128 + t * 32 + l31; swb[t] = (rowb[t] >> 2) & 3; }
    const uint32_t nk = dp / BH_BK;
    const float inv = 1.52587890625e-05f;    // 2^-16

    for (uint32_t c0 = 0; c0 < a.kc; c0 += BH_BN) {
        const uint64_t vleft = (uint64_t)(a.kc_pad - c0) * dp * 2;
        const __amdgpu_buffer_rsrc_t vres = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint16_t *>(a.c16 + (uint64_t)c0 * dp), 0, (int)(vleft > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)vleft), 0x00020000);
        auto fetch = [&](uint32_t k0) {
#pragma unroll
            for (int h = 0; h < 2; ++h) ra[h] = buf_ld16(qres, lane_b, k0 * 2 + h * r64_b);
#pragma unroll
            for (int h = 0; h < 4; ++h) rb[h] = buf_ld16(vres, lane_b, k0 * 2 + h * r64_b);
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int h = 0; h < 2; ++h) { const int r = ld_r + 64 * h; As4[buf][r * 4 + (ld_ch ^ ((r >> 2) & 3))] = ra[h]; }
#pragma unroll
            for (int h = 0; h < 4; ++h) { const int r = ld_r + 64 * h; Bs4[buf][r * 4 + (ld_ch ^ ((r >> 2) & 3))] = rb[h]; }
        };
        f32x16_t acc[2][4];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        fetch(0);
        stash(0);
        __syncthreads();
        for (uint32_t kt = 0; kt < nk; ++kt) {
            const int buf = (int)(kt & 1u);
            if (kt + 1 < nk) fetch((kt + 1) * BH_BK);
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                f16x8_t av[2], bv[4];
#pragma unroll
                for (int t = 0; t < 2; ++t) av[t] = __builtin_bit_cast(f16x8_t, As4[buf][rowa[t] * 4 + ((2 * j + lk) ^ swa[t])]);
#pragma unroll
                for (int t = 0; t < 4; ++t) bv[t] = __builtin_bit_cast(f16x8_t, Bs4[buf][rowb[t] * 4 + ((2 * j + lk) ^ swb[t])]);
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int jj = 0; jj < 4; ++jj)
                        acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(av[i], bv[jj], acc[i][jj], 0, 0, 0);
            }
            if (kt + 1 < nk) stash(buf ^ 1);
            __syncthreads();
        }
        // ---- bounds of this centroid tile.  C/D layout: col = lane & 31 (centroid), row = (r & 3) + 8 (r >> 2) + 4 lk
        float cn2[4], cs[4];
        bool cv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const uint32_t vj = c0 + wn * 128 + j * 32 + l31;
            cv[j] = vj < a.kc;
            cn2[j] = cv[j] ? a.cn2[vj] : 0.0f;
            cs[j] = sqrtf(cn2[j]) * 1.000001f;
        }
        auto bounds = [&](int i, int j, int r, float &lb, float &ub) {
            const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
            const float xn = xn2_s[ml], nn = xn + cn2[j];
            const float qv = xs_s[ml] * cs[j];                      // >= |a| |b|
            const float dt = nn - 2.0f * qv * (acc[i][j][r] * inv);
            const float err = 2.0f * qv * a.eps + 4.0e-6f * nn;
            ub = fmaxf(dt + err, 0.0f) * (1.0f + a.cm) + 1.0e-30f;
            lb = fmaxf(dt - err, 0.0f) * (1.0f - a.cm);
        };
        // (1) the rows' running thresholds: smallest upper bound of this tile, reduced over the 32 centroid lanes
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                float mn = INFINITY;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float lb, ub;
                    bounds(i, j, r, lb, ub);
                    if (cv[j] && ub < mn) mn = ub;                  // (a NaN bound never lowers a threshold)
                }
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) mn = fminf(mn, __shfl_xor(mn, off, 64));
                if (l31 == 0 && mn < INFINITY)
                    atomicMin(&thr_s[wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk], __float_as_uint(mn));
            }
        }
        __syncthreads();
        // (2) candidates: every centroid whose lower bound does not exceed its row's threshold (NaN bounds are kept)
#pragma unroll
        for (int i = 0; i < 2; ++i) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int ml = wm * 64 + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                const float thr = __uint_as_float(thr_s[ml]);
                const uint64_t row = m0 + ml;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    float lb, ub;
                    bounds(i, j, r, lb, ub);
                    if (cv[j] && row < a.m && !(lb > thr)) {
                        const uint32_t slot = atomicAdd(&a.cand_cnt[row], 1u);
                        if (slot < a.cap) a.cand[row * a.cap + slot] = c0 + wn * 128 + j * 32 + l31;
                    }
                }
            }
        }
        __syncthreads();          // the LDS stages are reused by the next centroid tile
    }
}
hipError_t launch_assign_f16(const AssignF16Args &a, hipStream_t s) {
    if (a.m == 0 || a.kc == 0) return hipSuccess;
    if ((a.dim_p % BH_BK) != 0 || (uint64_t)a.dim_p * 2 * 320 >= 0x7FFFFFFFull || (a.kc_pad % BH_BN) != 0 || a.kc_pad < a.kc)
        return hipErrorInvalidValue;
    const uint64_t blocks = (a.m + BH_BM - 1) / BH_BM;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assign_f16_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// exact pass: four lanes per row, each walking candidates 4 t + (lane & 3) of its row in the reference's order
__global__ __launch_bounds__(256) void assign_rescore_kernel(const float *__restrict__ rows, const float *__restrict__ centroids, uint64_t m,
                                                            uint32_t dim, uint32_t kc, const uint32_t *__restrict__ cand,
                                                            const uint32_t *__restrict__ cand_cnt, uint32_t cap, uint32_t *__restrict__ cluster) {
    const int lane = threadIdx.x & 63;
    const uint64_t row = ((uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6)) * 16 + (uint32_t)(lane >> 2);
    const uint32_t cl = (uint32_t)lane & 3u;
    const bool live = row < m;
    uint32_t cnt = live ? cand_cnt[row] : 0u;
    const bool all = cnt > cap;                       // list overflowed: every centroid is a candidate
    if (all) cnt = kc;
    const float *x = rows + (live ? row : 0) * dim;
    const uint32_t G = dim >> 2;
    uint64_t best = KEY_EMPTY;
    uint32_t rounds = (cnt + 3) >> 2;
    // (the loop count differs per lane: no cross-lane operation inside)
    for (uint32_t t = 0; t < rounds; ++t) {
        const uint32_t ci = 4 * t + cl;
        if (ci >= cnt) break;
        const uint32_t j = all ? ci : cand[row * cap + ci];
        const float *c = centroids + (uint64_t)j * dim;
        float sum = 0.0f;
        uint32_t g = 0;
        for (; g + 8 <= G; g += 8) {
            float4 xv[8], cvv[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) { xv[u] = load4<true>(x + (g + u) * 4); cvv[u] = load4<true>(c + (g + u) * 4); }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const float d0 = xv[u].x - cvv[u].x, d1 = xv[u].y - cvv[u].y, d2 = xv[u].z - cvv[u].z, d3 = xv[u].w - cvv[u].w;
                float tt = d0 * d0 + d1 * d1;
                tt = tt + d2 * d2;
                sum = sum + (tt + d3 * d3);
            }
        }
        for (; g < G; ++g) {
            const float4 xv = load4<true>(x + g * 4), cv = load4<true>(c + g * 4);
            const float d0 = xv.x - cv.x, d1 = xv.y - cv.y, d2 = xv.z - cv.z, d3 = xv.w - cv.w;
            float tt = d0 * d0 + d1 * d1;
            tt = tt + d2 * d2;
            sum = sum + (tt + d3 * d3);
        }
        const uint64_t key = ((uint64_t)__float_as_uint(sum) << 32) | j;
        best = key < best ? key : best;
    }
    // the row's four lanes: smallest (distance bits, index) = strict '<' in ascending centroid order (index.rs:408-415)
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) {
        const uint64_t o = shfl_u64(best, lane ^ off);
        best = o < best ? o : best;
    }
    if (live && cl == 0) cluster[row] = best == KEY_EMPTY ? 0u : (uint32_t)best;
}
// The same result with coalesced reads: a wave still owns 16 rows x 4 candidate slots per round, but the 64 lanes read one
// row (and each of its candidates' centroids) 1 KB at a time -- lane g computes the 4-group term of group g -- and park the
// terms in LDS [group][slot] (stride 65: conflict-free both ways); lane `slot` then adds its 64 terms in ascending group order,
// which is the reference's chain (index.rs:461-480).  A row is read once for its four slots.
__global__ __launch_bounds__(128) void assign_rescore_wave_kernel(const float *__restrict__ rows, const float *__restrict__ centroids, uint64_t m,
                                                                 uint32_t dim, uint32_t kc, const uint32_t *__restrict__ cand,
                                                                 const uint32_t *__restrict__ cand_cnt, uint32_t cap, uint32_t *__restrict__ cluster) {
    __shared__ float lds_all[2][64 * 65];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    float *lds = lds_all[wv];
    const uint64_t wave_row0 = ((uint64_t)blockIdx.x * 2 + (uint32_t)wv) * 16;
    const uint64_t row = wave_row0 + (uint32_t)(lane >> 2);
    const uint32_t cl = (uint32_t)lane & 3u;
    const bool live = row < m;
    uint32_t cnt = live ? cand_cnt[row] : 0u;
    const bool all = cnt > cap;                       // list overflowed: every centroid is a candidate
    if (all) cnt = kc;
    const uint32_t G = dim >> 2;
    uint64_t best = KEY_EMPTY;
    for (uint32_t t = 0;; ++t) {
        const uint32_t ci = 4 * t + cl;
        const bool act = ci < cnt;
        const uint64_t mask = __ballot(act);
        if (mask == 0) break;
        const uint32_t j = act ? (all ? ci : cand[row * cap + ci]) : 0u;
        float sum = 0.0f;
        for (uint32_t g0 = 0; g0 < G; g0 += 64) {
            const uint32_t ng = (G - g0 < 64u) ? (G - g0) : 64u;
            const bool gv = (uint32_t)lane < ng;
            const uint32_t goff = (g0 + (gv ? (uint32_t)lane : 0u)) * 4;
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                const uint32_t m4 = (uint32_t)(mask >> (4 * r)) & 0xFu;     // wave-uniform
                if (m4 == 0) continue;
                const float4 xv = load4<true>(rows + (wave_row0 + (uint32_t)r) * dim + goff);
                float4 cv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t jp = readlane_u32(j, 4 * r + u);
                    cv[u] = load4<true>(centroids + (uint64_t)jp * dim + goff);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d0 = xv.x - cv[u].x, d1 = xv.y - cv[u].y, d2 = xv.z - cv[u].z, d3 = xv.w - cv[u].w;
                    float tt = d0 * d0 + d1 * d1;
                    tt = tt + d2 * d2;
                    tt = tt + d3 * d3;
                    if (gv) lds[lane * 65 + 4 * r + u] = tt;
                }
            }
            wave_lds_fence();
            uint32_t e = 0;
            for (; e + 8 <= ng; e += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = lds[(e + u) * 65 + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u) sum = sum + v[u];
            }
            for (; e < ng; ++e) sum = sum + lds[e * 65 + lane];
            wave_lds_fence();
        }
        if (act) {
            const uint64_t key = ((uint64_t)__float_as_uint(sum) << 32) | j;
            best = key < best ? key : best;
        }
    }
    // the row's four lanes: smallest (distance bits, index) = strict '<' in ascending centroid order (index.rs:408-415)
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) {
        const uint64_t o = shfl_u64(best, lane ^ off);
        best = o < best ? o : best;
    }
    if (live && cl == 0) cluster[row] = best == KEY_EMPTY ? 0u : (uint32_t)best;
}
hipError_t launch_assign_rescore(const float *rows, const float *centroids, uint64_t m, uint32_t dim, uint32_t kc, const uint32_t *cand,
                                 const uint32_t *cand_cnt, uint32_t cap, uint32_t *cluster, hipStream_t s) {
    if (m == 0) return hipSuccess;
    if ((dim % 4) != 0) return hipErrorInvalidValue;
    // PQV_RESCORE_WAVE=0: the lane-per-(row, candidate) form above (A/B)
    static const bool wave_form = [] { const char *e = getenv("PQV_RESCORE_WAVE"); return !(e && *e == '0'); }();
    if (wave_form && dim >= 64) {
        const uint64_t wblocks = (m + 31) / 32;
        if (wblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        hipLaunchKernelGGL(assign_rescore_wave_kernel, dim3((uint32_t)wblocks), dim3(128), 0, s, rows, centroids, m, dim, kc, cand, cand_cnt, cap, cluster);
        return hipGetLastError();
    }
    const uint64_t blocks = (m + 63) / 64;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assign_rescore_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, centroids, m, dim, kc, cand, cand_cnt, cap, cluster);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Round 4: assign_wide_kernel + assign_resolve_kernel (see kernels.h: AssignWideArgs).
//
// Block = 256 rows against ALL centroids, 256 at a time; 8 waves as 2 (centroid side, M) x 4 (row side, N), each 128 centroids
// x 64 rows = 4 x 2 tiles of v_mfma_f32_32x32x16_f16; K in 128-byte stages through double-buffered, chunk-swizzled LDS
// (brute_f16_kernel's loop).  C/D layout: col = lane & 31 is the N index -- a DATA ROW --, the 16 registers of a tile are
// centroids (r & 3) + 8 (r >> 2) + 4 (lane >> 5).  A lane therefore owns two rows and sees 64 of a tile's 256 centroids for each.
//   t_c   = cn2[c] - kA xs acc            (d~ = |x - mu|^2 + t_c;  |d~ - d| <= E = 2 xs cmaxs eps + 4e-6 (|x - mu|^2 + cn_max))
//   best  = min_c t_c                     lane-local over 64 registers, one cross-half shuffle, one LDS atomicMin per wave pair
//   keep  <=> !(t_c > cut(best))          cut: assign_cut below -- every centroid whose reference distance could be <= the
//                                         reference distance of the best one (ties included: the lowest index must win)
// The test runs per lane on its own minimum first; only a lane that holds a candidate walks its 64 registers.
// ------------------------------------------------------------------------------------
// cut for the candidates' LOWER-bound scores, from the row's smallest UPPER-bound score `ub_best` (scores: d~ - |x - mu|^2 -+ E):
// U >= the reference distance of the best centroid; c can only matter if (d~_c - E_c)(1 - cm) <= U, i.e. (t_c - E_c) <= cut
__device__ __forceinline__ float assign_cut(float xn, float ub_best, float cm) {
    const float U = fmaxf(xn + ub_best, 0.0f) * (1.0f + cm) + 1.0e-30f;
    const float cut = U / (1.0f - cm) - xn;
    return cut + 4.0e-6f * (fabsf(U) + xn) + 1.0e-30f;          // the f32 roundings of this expression, upward
}

constexpr int AW_TM = 4, AW_TN = 2, AW_NWM = 2, AW_NWN = 4, AW_ST = 8;
constexpr int AW_BM = 32 * AW_TM * AW_NWM, AW_BN = 32 * AW_TN * AW_NWN, AW_NT = 64 * AW_NWM * AW_NWN;     // 256 centroids x 256 rows, 512 threads
// <NWN, ST>: <4, 8> = the 256 x 256 tile, eight waves, 128-byte K stages, ONE block per CU (the default);
// <2, 4> (round 6, PQV_ASSIGN_SHAPE=128): 256 centroids x 128 rows, four waves of the same 128 x 64 shape, 64-byte stages -- 48 KB of LDS,
// TWO blocks per CU, so that one block's epilogue (its CU otherwise idle: 20 % of a centroid tile) runs under the other's K loop
template <int NWN, int ST>
__global__ __launch_bounds__(64 * AW_NWM * NWN, NWN == 4 ? 1 : 2) void assign_wide_kernel(const AssignWideArgs a) {
    constexpr int TM = AW_TM, TN = AW_TN, BM = AW_BM, BN = 32 * AW_TN * NWN, NT = 64 * AW_NWM * NWN;
    constexpr int CA = BM * ST / NT, CB = BN * ST / NT;        // 16-byte chunks a thread stages per K stage and side
    extern __shared__ float4 aw_lds[];                         // [2][BM * ST] centroid stages, [2][BN * ST] row stages
    float4 *const As4 = aw_lds, *const Bs4 = aw_lds + 2 * BM * ST;
    auto sw = [](int r) { return ST == 4 ? (r >> 2) & 3 : ((r >> 1) & 1) | (((r >> 2) & 3) << 1); };      // 64- / 128-byte rows: brute_f16_kernel's swizzles
    __shared__ float cn_s[BM];               // cn2 of the current centroid tile (+inf beyond kc)
    __shared__ float gcs_s[BM / 32], gcn_s[BM / 32];      // per 32-centroid group of the tile: >= max |c - mu|, >= max cn2
    __shared__ uint32_t best_s[BN];          // sortable bits of the rows' smallest upper-bound score so far

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const uint64_t n0 = (uint64_t)blockIdx.x * BN;             // first data row of the block
    const uint32_t rbytes = a.dim_p * 2;
    constexpr int RPS = NT / ST;
    const int ld_r = tid / ST, ld_ch = tid % ST;
    float4 ra[CA], rb[CB];
    const uint64_t vleft = (a.m - n0) * rbytes;
    const __amdgpu_buffer_rsrc_t vres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t *>(a.x16 + n0 * a.dim_p), 0, (int)(vleft > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)vleft), 0x00020000);
    const uint32_t lane_b = (uint32_t)ld_r * rbytes + (uint32_t)ld_ch * 16, step_b = (uint32_t)RPS * rbytes;
    if (tid < BN) best_s[tid] = 0xFFFFFFFFu;

    const int l31 = lane & 31, lk = lane >> 5;
    int rowa[TM], rowb[TN], swa[TM], swb[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) { rowa[t] = wm * 32 * TM + t * 32 + l31; swa[t] = sw(rowa[t]); }
#pragma unroll
    for (int t = 0; t < TN; ++t) { rowb[t] = wn * 32 * TN + t * 32 + l31; swb[t] = sw(rowb[t]); }
    // the lane's two rows
    float xn[TN], xs2e[TN], Ar[TN];
    uint64_t grow[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) {
        grow[j] = n0 + (uint64_t)rowb[j];
        xn[j] = grow[j] < a.m ? a.xn2[grow[j]] : 0.0f;
        const float xs = sqrtf(xn[j]) * 1.000001f;
        xs2e[j] = 2.0f * xs * a.eps;
        Ar[j] = xs * a.kA;
    }
    const uint32_t nk = rbytes / (16 * ST);

    for (uint32_t c0 = 0; c0 < a.kc; c0 += BM) {
        const uint64_t qleft = (uint64_t)(a.kc_pad - c0) * rbytes;
        const __amdgpu_buffer_rsrc_t qres = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint16_t *>(a.c16 + (uint64_t)c0 * a.dim_p), 0, (int)(qleft > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)qleft), 0x00020000);
        auto fetch = [&](uint32_t kb) {
#pragma unroll
            for (int h = 0; h < CA; ++h) ra[h] = buf_ld16(qres, lane_b, kb + h * step_b);
#pragma unroll
            for (int h = 0; h < CB; ++h) rb[h] = buf_ld16(vres, lane_b, kb + h * step_b);
        };
        auto stash = [&](int buf) {
#pragma unroll
            for (int h = 0; h < CA; ++h) { const int r = ld_r + RPS * h; As4[buf * BM * ST + r * ST + (ld_ch ^ sw(r))] = ra[h]; }
#pragma unroll
            for (int h = 0; h < CB; ++h) { const int r = ld_r + RPS * h; Bs4[buf * BN * ST + r * ST + (ld_ch ^ sw(r))] = rb[h]; }
        };
        if (tid < BM) cn_s[tid] = c0 + tid < a.kc ? a.cn2[c0 + tid] : INFINITY;
        if (tid < BM / 32) { gcs_s[tid] = a.grp_cs[c0 / 32 + tid]; gcn_s[tid] = a.grp_cn[c0 / 32 + tid]; }
        f32x16_t acc[TM][TN];
#pragma unroll
        for (int i = 0; i < TM; ++i)
#pragma unroll
            for (int j = 0; j < TN; ++j)
#pragma unroll
                for (int r = 0; r < 16; ++r) acc[i][j][r] = 0.0f;
        fetch(0);
        stash(0);
        __syncthreads();
        for (uint32_t kt = 0; kt < nk; ++kt) {
            const int buf = (int)(kt & 1u);
            if (kt + 1 < nk) fetch((kt + 1) * 16 * ST);
            float4 av[2][TM], bv[2][TN];
            auto lds_read = [&](int j, int set) {
#pragma unroll
                for (int t = 0; t < TM; ++t) av[set][t] = As4[buf * BM * ST + rowa[t] * ST + ((2 * j + lk) ^ swa[t])];
#pragma unroll
                for (int t = 0; t < TN; ++t) bv[set][t] = Bs4[buf * BN * ST + rowb[t] * ST + ((2 * j + lk) ^ swb[t])];
            };
            lds_read(0, 0);
#pragma unroll
            for (int j = 0; j < ST / 2; ++j) {
                const int set = j & 1;
                if (j + 1 < ST / 2) lds_read(j + 1, set ^ 1);
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int i = 0; i < TM; ++i)
#pragma unroll
                    for (int jj = 0; jj < TN; ++jj)
                        acc[i][jj] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, av[set][i]), __builtin_bit_cast(f16x8_t, bv[set][jj]), acc[i][jj], 0, 0, 0);
                __builtin_amdgcn_sched_barrier(0);
            }
            if (kt + 1 < nk) stash(buf ^ 1);
            __syncthreads();
        }
        // ---- pass 1: t in place of the accumulators; per 32-centroid group the error term E (the centroids are sorted by norm:
        // a group's own maximum, not the table's, scales its bound), the lane's smallest upper- and lower-bound scores per row
        float mub[TN], mlb[TN], Eg[TM][TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) { mub[j] = INFINITY; mlb[j] = INFINITY; }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float gcs = gcs_s[wm * TM + i], gcn = gcn_s[wm * TM + i];
            float mt[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) { Eg[i][j] = xs2e[j] * gcs + 4.0e-6f * (xn[j] + gcn); mt[j] = INFINITY; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float cn = cn_s[wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk];
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const float t = __builtin_fmaf(-Ar[j], acc[i][j][r], cn);
                    acc[i][j][r] = t;
                    mt[j] = fminf(mt[j], t);
                }
            }
#pragma unroll
            for (int j = 0; j < TN; ++j) { mub[j] = fminf(mub[j], mt[j] + Eg[i][j]); mlb[j] = fminf(mlb[j], mt[j] - Eg[i][j]); }
        }
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const float m2 = fminf(mub[j], __shfl_xor(mub[j], 32, 64));
            if (lk == 0 && m2 < INFINITY) atomicMin(&best_s[rowb[j]], sortable_bits(m2));
        }
        __syncthreads();
        // ---- pass 2: candidates against the best so far (their lower-bound scores travel with them)
#pragma unroll
        for (int j = 0; j < TN; ++j) {
            const uint32_t bb = best_s[rowb[j]];
            const float cut = assign_cut(xn[j], bb == 0xFFFFFFFFu ? INFINITY : unsortable_bits(bb), a.cm);
            if (grow[j] < a.m && !(mlb[j] > cut)) {
#pragma unroll
                for (int i = 0; i < TM; ++i) {
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const float tl = acc[i][j][r] - Eg[i][j];
                        if (!(tl > cut)) {
                            const uint32_t slot = atomicAdd(&a.cand_cnt[grow[j]], 1u);
                            if (slot < a.cap) {
                                a.cand[grow[j] * a.cap + slot] = c0 + wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk;
                                a.cand_t[grow[j] * a.cap + slot] = tl;
                            }
                        }
                    }
                }
            }
        }
        __syncthreads();          // cn_s, the group tables and the LDS stages are rewritten by the next centroid tile
    }
    if (tid < BN && n0 + tid < a.m) {
        const uint32_t bb = best_s[tid];
        a.best_t[n0 + tid] = bb == 0xFFFFFFFFu ? INFINITY : unsortable_bits(bb);
    }
}
hipError_t launch_assign_wide(const AssignWideArgs &a, hipStream_t s) {
    if (a.m == 0 || a.kc == 0) return hipSuccess;
    if ((a.dim_p % 64) != 0 || (uint64_t)a.dim_p * 2 * 512 >= 0x7FFFFFFFull || (a.kc_pad % AW_BM) != 0 || a.kc_pad < a.kc) return hipErrorInvalidValue;
    // 256 centroids x 128 rows in 4-wave blocks, two per CU, where the rows make fewer than two rounds of 256-row blocks (the Lloyd
    // iterations over the 100 k sample: 16.2-16.5 against 17.1-17.3 ms for twenty of them); PQV_ASSIGN_SHAPE=128 / 256 forces a shape
    static const int shape = [] { const char *e = getenv("PQV_ASSIGN_SHAPE"); return e ? atoi(e) : 0; }();
    const bool half = shape == 128 || (shape != 256 && a.m < 2ull * 256 * AW_BN);
    if (half) {
        constexpr int BN = 32 * AW_TN * 2;
        const uint64_t blocks = (a.m + BN - 1) / BN;
        if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
        constexpr size_t lds = 2 * (size_t)(AW_BM + BN) * 4 * 16;
        hipLaunchKernelGGL((assign_wide_kernel<2, 4>), dim3((uint32_t)blocks), dim3(256), lds, s, a);
        return hipGetLastError();
    }
    const uint64_t blocks = (a.m + AW_BN - 1) / AW_BN;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    constexpr size_t lds = 2 * (size_t)(AW_BM + AW_BN) * AW_ST * 16;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(assign_wide_kernel<AW_NWN, AW_ST>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    hipLaunchKernelGGL((assign_wide_kernel<AW_NWN, AW_ST>), dim3((uint32_t)blocks), dim3(AW_NT), lds, s, a);
    return hipGetLastError();
}

// The second half: a wave owns 16 rows x 4 candidate slots per round (assign_rescore_wave_kernel's tiling).  A row's candidates
// are first filtered against the row's FINAL best; a row left with one survivor is done -- its f32 row is never read -- and
// only rows with two or more (or an overflowed list: every centroid) go through the exact chains.
__global__ __launch_bounds__(128) void assign_resolve_kernel(const AssignWideArgs a, const float *__restrict__ rows, const float *__restrict__ centroids,
                                                            uint32_t dim, uint32_t *__restrict__ cluster, unsigned long long *__restrict__ stats) {
    __shared__ float lds_all[2][64 * 65];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    float *lds = lds_all[wv];
    const uint64_t wave_row0 = ((uint64_t)blockIdx.x * 2 + (uint32_t)wv) * 16;
    const uint64_t row = wave_row0 + (uint32_t)(lane >> 2);
    const uint32_t cl = (uint32_t)lane & 3u;
    const bool live = row < a.m;
    uint32_t cnt = live ? a.cand_cnt[row] : 0u;
    const bool all = cnt > a.cap;                     // list overflowed: every centroid is a candidate
    float cut = INFINITY;
    if (live && !all) {
        cut = assign_cut(a.xn2[row], a.best_t[row], a.cm);
    }
    // survivors of the row: count and (where it is the only one) the id
    uint32_t nsurv = 0, only = 0;
    if (!all)
        for (uint32_t ci = cl; ci < cnt; ci += 4)
            if (!(a.cand_t[row * a.cap + ci] > cut)) { ++nsurv; only = a.perm[a.cand[row * a.cap + ci]]; }
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) {
        const uint32_t on = (uint32_t)__shfl_xor((int)nsurv, off, 64), oo = (uint32_t)__shfl_xor((int)only, off, 64);
        only = nsurv ? only : oo;          // (meaningful only when the total is 1)
        nsurv += on;
    }
    const bool exact = live && (all || nsurv != 1u);
    if (all) cnt = a.kc;
    if (!exact) cnt = 0;
    const uint32_t G = dim >> 2;
    uint64_t best = KEY_EMPTY;
    uint32_t n_eval = 0;
    for (uint32_t t = 0;; ++t) {
        const uint32_t ci = 4 * t + cl;
        bool act = ci < cnt;
        uint32_t j = 0u;
        if (act) {
            if (all) j = ci;
            else { j = a.perm[a.cand[row * a.cap + ci]]; act = !(a.cand_t[row * a.cap + ci] > cut); }
        }
        if (__ballot(ci < cnt) == 0) break;
        const uint64_t mask = __ballot(act);
        if (mask == 0) continue;
        n_eval += act ? 1u : 0u;
        float sum = 0.0f;
        for (uint32_t g0 = 0; g0 < G; g0 += 64) {
            const uint32_t ng = (G - g0 < 64u) ? (G - g0) : 64u;
            const bool gv = (uint32_t)lane < ng;
            const uint32_t goff = (g0 + (gv ? (uint32_t)lane : 0u)) * 4;
#pragma unroll 1
            for (int r = 0; r < 16; ++r) {
                const uint32_t m4 = (uint32_t)(mask >> (4 * r)) & 0xFu;     // wave-uniform
                if (m4 == 0) continue;
                const float4 xv = load4<true>(rows + (wave_row0 + (uint32_t)r) * dim + goff);
                float4 cv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t jp = readlane_u32(j, 4 * r + u);
                    cv[u] = load4<true>(centroids + (uint64_t)jp * dim + goff);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float d0 = xv.x - cv[u].x, d1 = xv.y - cv[u].y, d2 = xv.z - cv[u].z, d3 = xv.w - cv[u].w;
                    float tt = d0 * d0 + d1 * d1;
                    tt = tt + d2 * d2;
                    tt = tt + d3 * d3;
                    if (gv) lds[lane * 65 + 4 * r + u] = tt;
                }
            }
            wave_lds_fence();
            uint32_t e = 0;
            for (; e + 8 <= ng; e += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = lds[(e + u) * 65 + lane];
#pragma unroll
                for (int u = 0; u < 8; ++u) sum = sum + v[u];
            }
            for (; e < ng; ++e) sum = sum + lds[e * 65 + lane];
            wave_lds_fence();
        }
        if (act) {
            const uint64_t key = ((uint64_t)__float_as_uint(sum) << 32) | j;
            best = key < best ? key : best;
        }
    }
    // the row's four lanes: smallest (distance bits, index) = strict '<' in ascending centroid order (index.rs:408-415)
#pragma unroll
    for (int off = 1; off < 4; off <<= 1) {
        const uint64_t o = shfl_u64(best, lane ^ off);
        best = o < best ? o : best;
    }
    if (live && cl == 0) cluster[row] = exact ? (best == KEY_EMPTY ? 0u : (uint32_t)best) : only;
    if (stats) {
        const unsigned long long rows_x = (unsigned long long)__popcll(__ballot(exact && cl == 0));
        uint32_t ev = n_eval;
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) ev += (uint32_t)__shfl_xor((int)ev, off, 64);
        if (lane == 0 && (rows_x || ev)) { atomicAdd(&stats[0], rows_x); atomicAdd(&stats[1], (unsigned long long)ev); }
    }
}
hipError_t launch_assign_resolve(const AssignWideArgs &a, const float *rows, const float *centroids, uint32_t dim, uint32_t *cluster,
                                 unsigned long long *stats, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    if ((dim % 4) != 0) return hipErrorInvalidValue;
    const uint64_t wblocks = (a.m + 31) / 32;
    if (wblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assign_resolve_kernel, dim3((uint32_t)wblocks), dim3(128), 0, s, a, rows, centroids, dim, cluster, stats);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// k-means++ rounds with an int8 screen (kernels.h: MinUpdScreenArgs).  One wave per 16-row tile.
//   screen   A = the picked row's image (every M row the same: an LDS broadcast), B = the tile's images straight from global
//            memory (one contiguous 1 KiB per K step of 64 dims): lane (l15, kk) ends with the image dot product of row l15 in
//            every accumulator register; |xi - ci|^2 = Nx + Nc - 2 dot is exact, and
//                ref(x, c) >= (max(0, sqrt(|xi - ci|^2) / S - rx - rc))^2 (1 - cm)          (block_rows_i8_kernel's residual bounds)
//   exact    rows the bound cannot rule out: the wave reads such a row 1 KiB at a time, lane g forms the 4-group term of group
//            g (index.rs:466-472), parks it in LDS [group][row slot], and lane `slot` adds its row's terms in ascending group
//            order -- the reference's chain, as in stream_kernel.
// ------------------------------------------------------------------------------------
// one 16-row tile of a round: screen + exact evaluation of what it cannot rule out
__device__ __forceinline__ void minupd_screen_tile(const MinUpdScreenArgs &a, uint64_t pick, uint64_t T, const float4 *cimg, float *terms, int lane) {
    const uint32_t dim = a.dim, G16 = dim >> 4, G = dim >> 2;
    const int l15 = lane & 15, kk = lane >> 4;
    // ---- screen: image dot products of the tile's 16 rows with the picked row
    const float4 *tb = a.img + T * G16 * 16;
    i32x4_acc acc = {0, 0, 0, 0};
    const uint32_t nks = G16 >> 2;                   // K steps of 64 dims
    constexpr int NB = 12;                           // operand loads in flight
    for (uint32_t k0 = 0; k0 < nks; k0 += NB) {
        float4 xb[NB];
#pragma unroll
        for (int u = 0; u < NB; ++u) {
            const uint32_t ks = k0 + u < nks ? k0 + u : nks - 1;
            xb[u] = tb[ks * 64 + lane];
        }
#pragma unroll
        for (int u = 0; u < NB; ++u)
            if (k0 + u < nks) mfma_step<OP_I8>(acc, cimg[4 * (k0 + u) + kk], xb[u]);
    }
    const uint64_t row = T * 16 + (uint32_t)l15;
    const bool live = row < a.n;
    const int nc = a.n2i[pick];
    const float rc = a.res[pick];
    const int nx = live ? a.n2i[row] : 0;
    const float rx = live ? a.res[row] : 0.0f;
    const float old = live ? a.min_d[row] : 0.0f;
    // |xi - ci|^2: exact in int32 (<= 4 * 127^2 dim); its f32 image and square root are rounded DOWNWARD by the factors below
    const int di = nx + nc - 2 * acc[0];
    const float dn = sqrtf((float)(di > 0 ? di : 0)) * 0.999999f * a.inv_s;
    const float g = fmaxf(dn * 0.999999f - (rx + rc) * 1.000001f, 0.0f);
    const float lb = g * g * 0.999999f * (1.0f - a.cm);
    const bool need = live && kk == 0 && !(lb > old);       // (a NaN bound is never a reason to skip)
    const uint64_t mask = __ballot(need);                    // bits 0..15: rows of the tile to evaluate exactly
    if (mask == 0) return;
    // ---- exact distances of the flagged rows, the reference's order
    const float *crow = a.rows + pick * dim;
    float sum = 0.0f;
    for (uint32_t c0 = 0; c0 < G; c0 += 64) {
        const uint32_t ng = G - c0 < 64u ? G - c0 : 64u;
        const bool gv = (uint32_t)lane < ng;
        const uint32_t goff = (c0 + (gv ? (uint32_t)lane : 0u)) * 4;
        const float4 qq = load4<true>(crow + goff);
        uint64_t todo = mask;
        while (todo) {
            // up to four rows' loads in flight
            int sl[4];
            float4 xv[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                sl[u] = todo ? __builtin_ctzll(todo) : -1;
                if (todo) todo &= todo - 1;
                if (sl[u] >= 0) xv[u] = load4<true>(a.rows + (T * 16 + (uint32_t)sl[u]) * dim + goff);
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (sl[u] < 0) continue;
                const float d0 = qq.x - xv[u].x, d1 = qq.y - xv[u].y, d2 = qq.z - xv[u].z, d3 = qq.w - xv[u].w;
                float t = d0 * d0 + d1 * d1;
                t = t + d2 * d2;
                t = t + d3 * d3;
                if (gv) terms[lane * 17 + sl[u]] = t;
            }
        }
        wave_lds_fence();
        if (need) {
            uint32_t e = 0;
            for (; e + 8 <= ng; e += 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u) v[u] = terms[(e + u) * 17 + l15];
#pragma unroll
                for (int u = 0; u < 8; ++u) sum = sum + v[u];
            }
            for (; e < ng; ++e) sum = sum + terms[e * 17 + l15];
        }
        wave_lds_fence();
    }
    if (need && sum < old) {                                 // index.rs:363-365
        a.min_d[row] = sum;
        if (a.mirror) a.mirror[row] = sum;
        if (a.mirror_t) a.mirror_t[(row % a.mirror_chunk) * a.mirror_stride + row / a.mirror_chunk] = sum;
    }
}
__global__ __launch_bounds__(256) void minupd_screen_kernel(const MinUpdScreenArgs a) {
    extern __shared__ float4 mus_lds[];              // [G16] the picked row's image, then per wave [64][17] floats of chain terms
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t G16 = a.dim >> 4;
    float4 *cimg = mus_lds;
    float *terms = reinterpret_cast<float *>(mus_lds + G16) + wave * (64 * 17);
    if (a.stop && *a.stop) return;                   // (the rounds enqueued ahead: an earlier one went back to the host)
    const uint64_t pick = a.pick_dev ? (uint64_t)*a.pick_dev : a.pick;
    if (pick >= a.n) return;
    {
        const uint64_t Tp = pick >> 4, jp = pick & 15;
        for (uint32_t cc = threadIdx.x; cc < G16; cc += 256) cimg[cc] = a.img[(Tp * G16 + cc) * 16 + jp];
    }
    __syncthreads();
    const uint64_t n_tiles = (a.n + 15) >> 4;
    const uint64_t T = (uint64_t)blockIdx.x * 4 + (uint32_t)wave;
    if (T < n_tiles) minupd_screen_tile(a, pick, T, cimg, terms, lane);
}
hipError_t launch_minupd_screen(const MinUpdScreenArgs &a, hipStream_t s) {
    if (a.n == 0) return hipSuccess;
    if ((a.dim % 64) != 0 || (!a.pick_dev && a.pick >= a.n)) return hipErrorInvalidValue;
    const uint64_t n_tiles = (a.n + 15) / 16, blocks = (n_tiles + 3) / 4;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    const size_t lds = (size_t)(a.dim / 16) * 16 + 4 * 64 * 17 * sizeof(float);
    if (lds > 65536) return hipErrorInvalidValue;
    hipLaunchKernelGGL(minupd_screen_kernel, dim3((uint32_t)blocks), dim3(256), lds, s, a);
    return hipGetLastError();
}

// |row - mu|^2 and 1 / |row - mu| per row, and the f16 image of (row - mu) / |row - mu| * 2^8 zero-padded to dim_p:
// one wave per row (mu == nullptr: no centring).  pad_to rows beyond n are written as zero rows (the centroid table is
// padded to a multiple of 256 rows).
__global__ __launch_bounds__(256) void center_normalize_f16_kernel(const float *__restrict__ rows, const float *__restrict__ mu, uint64_t n,
                                                                  uint64_t n_pad, uint32_t dim, uint32_t dim_p, float *__restrict__ out_n2,
                                                                  uint16_t *__restrict__ out, float fixed_scale, const uint32_t *__restrict__ idx) {
    const int lane = threadIdx.x & 63;
    const uint64_t w = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t nw = (uint64_t)gridDim.x * 4;
    for (uint64_t r = w; r < n_pad; r += nw) {
        if (r >= n) {
            for (uint32_t e = lane; e < dim_p; e += 64) out[r * dim_p + e] = 0;
            continue;
        }
        const float *p = rows + (idx ? (uint64_t)idx[r] : r) * dim;
        float acc = 0.0f;
        if ((dim & 7u) == 0 && dim <= 2048) {
            // 8 values (two 16-byte loads) per lane and step, kept in registers between the norm and the scaling pass
            float4 v[4][2];
            const uint32_t G8 = dim >> 3;
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t g = (uint32_t)lane + 64u * (uint32_t)u;
                if (g < G8) {
                    const float4 *pp = reinterpret_cast<const float4 *>(p + g * 8);
                    float4 a0 = pp[0], a1 = pp[1];
                    if (mu) {
                        const float4 *mm = reinterpret_cast<const float4 *>(mu + g * 8);
                        const float4 m0 = mm[0], m1 = mm[1];
                        a0.x -= m0.x; a0.y -= m0.y; a0.z -= m0.z; a0.w -= m0.w; a1.x -= m1.x; a1.y -= m1.y; a1.z -= m1.z; a1.w -= m1.w;
                    }
                    v[u][0] = a0; v[u][1] = a1;
                    acc = fmaf(a0.x, a0.x, acc); acc = fmaf(a0.y, a0.y, acc); acc = fmaf(a0.z, a0.z, acc); acc = fmaf(a0.w, a0.w, acc);
                    acc = fmaf(a1.x, a1.x, acc); acc = fmaf(a1.y, a1.y, acc); acc = fmaf(a1.z, a1.z, acc); acc = fmaf(a1.w, a1.w, acc);
                }
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
            if (lane == 0) out_n2[r] = acc;
            const float sc = fixed_scale > 0.0f ? fixed_scale : acc > 0.0f ? 256.0f / sqrtf(acc) : 0.0f;
            auto cl = [&](float x) { return fminf(fmaxf(x * sc, -65504.0f), 65504.0f); };
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const uint32_t g = (uint32_t)lane + 64u * (uint32_t)u;
                if (g < (dim_p >> 3)) {
                    f16x8_t h = {0, 0, 0, 0, 0, 0, 0, 0};
                    if (g < G8) {
                        h[0] = (_Float16)cl(v[u][0].x); h[1] = (_Float16)cl(v[u][0].y); h[2] = (_Float16)cl(v[u][0].z); h[3] = (_Float16)cl(v[u][0].w);
                        h[4] = (_Float16)cl(v[u][1].x); h[5] = (_Float16)cl(v[u][1].y); h[6] = (_Float16)cl(v[u][1].z); h[7] = (_Float16)cl(v[u][1].w);
                    }
                    *reinterpret_cast<float4 *>(out + r * dim_p + g * 8) = __builtin_bit_cast(float4, h);
                }
            }
            continue;
        }
        for (uint32_t e = lane; e < dim; e += 64) { const float v = p[e] - (mu ? mu[e] : 0.0f); acc = fmaf(v, v, acc); }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off, 64);
        if (lane == 0) out_n2[r] = acc;
        const float sc = fixed_scale > 0.0f ? fixed_scale : acc > 0.0f ? 256.0f / sqrtf(acc) : 0.0f;
        for (uint32_t e = lane; e < dim_p; e += 64) {
            float v = e < dim ? (p[e] - (mu ? mu[e] : 0.0f)) * sc : 0.0f;
            v = fminf(fmaxf(v, -65504.0f), 65504.0f);
            const _Float16 h = (_Float16)v;
            out[r * dim_p + e] = __builtin_bit_cast(uint16_t, h);
        }
    }
}
hipError_t launch_center_normalize_f16(const float *rows, const float *mu, uint64_t n, uint64_t n_pad, uint32_t dim, uint32_t dim_p,
                                       float *out_n2, void *out, hipStream_t s, float fixed_scale, const uint32_t *idx) {
    if (n_pad == 0) return hipSuccess;
    uint64_t blocks = (n_pad + 3) / 4;
    if (blocks > 65536) blocks = 65536;
    hipLaunchKernelGGL(center_normalize_f16_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rows, mu, n, n_pad, dim, dim_p, out_n2,
                       static_cast<uint16_t *>(out), fixed_scale, idx);
    return hipGetLastError();
}
// (follows center_normalize_f16_kernel's two summation loops: change them together)
uint32_t center_normalize_f16_sum_depth(uint32_t dim) {
    const uint32_t per_lane = ((dim & 7u) == 0 && dim <= 2048) ? 8u * ((dim / 8u + 63u) / 64u) : (dim + 63u) / 64u;
    return per_lane + 6u;
}
// mu[d] = mean over the k rows of m[., d]: one block per 64 columns, SIXTEEN row slices per column (four loads in flight each)
// reduced through LDS.  (mu only centres the f16 images of the assignment -- the bounds hold for any mu --, so the order of this
// sum is free; with four slices of 256 dependent loads it was 80 us of every Lloyd iteration.)
__global__ __launch_bounds__(1024) void col_mean_kernel(const float *__restrict__ m, uint32_t k, uint32_t dim, float *__restrict__ mu) {
    __shared__ float part[16][64];
    const uint32_t lane = threadIdx.x & 63u, d = blockIdx.x * 64u + lane, sl = threadIdx.x >> 6;
    float acc = 0.0f;
    if (d < dim) {
        uint32_t r = sl;
        for (; r + 48 < k; r += 64) {
            const float v0 = m[(uint64_t)r * dim + d], v1 = m[(uint64_t)(r + 16) * dim + d];
            const float v2 = m[(uint64_t)(r + 32) * dim + d], v3 = m[(uint64_t)(r + 48) * dim + d];
            acc += (v0 + v1) + (v2 + v3);
        }
        for (; r < k; r += 16) acc += m[(uint64_t)r * dim + d];
    }
    part[sl][lane] = acc;
    __syncthreads();
    if (sl == 0 && d < dim) {
        float t = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) t += part[i][lane];
        mu[d] = k ? t / (float)k : 0.0f;
    }
}
hipError_t launch_col_mean(const float *m, uint32_t k, uint32_t dim, float *mu, hipStream_t s) {
    if (dim == 0) return hipSuccess;
    hipLaunchKernelGGL(col_mean_kernel, dim3((dim + 63) / 64), dim3(1024), 0, s, m, k, dim, mu);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// Helpers of the MFMA-screened assignment (api.cpp: assign_screened): the k-means assignment of a
// chunk of rows is the top-1 search of every row among the centroids, i.e. the wide screened path
// with the rows as queries and ONE list holding all centroids.
//   assign_setup_kernel : identity bucketing (pair i = query i, quads of `width` consecutive queries of
//                         cluster 0), candidate bases 0, thresholds EMPTY
//   nonfinite_flag_kernel / count_changed_kernel : see the launchers' comments in kernels.h
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void assign_setup_kernel(uint32_t *pairs, uint4 *quads, uint32_t *n_quads, uint64_t *cand_base,
                                                          unsigned long long *gthr, uint32_t nq, uint32_t width) {
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    if (i == 0) *n_quads = (nq + width - 1) / width;
    if (i >= nq) return;
    pairs[i] = i;
    cand_base[i] = 0;
    gthr[i] = ~0ull;
    if (i % width == 0) quads[i / width] = make_uint4(0u, i, nq - i < width ? nq - i : width, 0u);
}
hipError_t launch_assign_setup(uint32_t *pairs, uint4 *quads, uint32_t *n_quads, uint64_t *cand_base, unsigned long long *gthr,
                               uint32_t nq, uint32_t width, hipStream_t s) {
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(assign_setup_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, pairs, quads, n_quads, cand_base, gthr, nq, width);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void nonfinite_flag_kernel(const float *v, uint64_t n, uint32_t *flag) {
    bool bad = false;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) bad |= !(fabsf(v[i]) < INFINITY);
    if (__ballot(bad) != 0ull && (threadIdx.x & 63) == 0) atomicOr(flag, 1u);
}
hipError_t launch_nonfinite_flag(const float *v, uint64_t n, uint32_t *flag, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(nonfinite_flag_kernel, dim3((uint32_t)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, v, n, flag);
    return hipGetLastError();
}
__global__ __launch_bounds__(256) void count_changed_kernel(const uint32_t *cur, const uint32_t *prev, uint64_t n,
                                                           unsigned long long *changed) {
    uint32_t c = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256) c += cur[i] != prev[i];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) c += (uint32_t)__shfl_down((int)c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(changed, (unsigned long long)c);
}
hipError_t launch_count_changed(const uint32_t *cur, const uint32_t *prev, uint64_t n, unsigned long long *changed, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    hipLaunchKernelGGL(count_changed_kernel, dim3((uint32_t)(blocks < 2048 ? blocks : 2048)), dim3(256), 0, s, cur, prev, n, changed);
    return hipGetLastError();
}


// ------------------------------------------------------------------------------------
// Round 6: the inverted lists on the device -- a stable counting sort of the rows by cluster (index.rs:193-206: list c = the row ids
// assigned to c in ASCENDING order, as the sequential scan pushes them).  Three launches:
//   list_hist_kernel     block b counts the clusters of its rows_per_block consecutive rows (LDS), cnt[c][b] = count
//   list_scan_kernel     block c turns cnt[c][.] into exclusive prefixes over the blocks and leaves the cluster's total in tot[c];
//   list_offsets_kernel  one block: list_off = exclusive scan of tot (u64), list_off[k] = n
//   list_scatter_kernel  block b again: wave w takes the w-th quarter of the block's rows, 64 at a time in row order; a row's slot is
//                        list_off[c] + (rows of c in earlier blocks) + (in earlier waves of this block) + (earlier in this wave):
//                        blocks, waves, steps and lanes are all walked in row order, so every list comes out ascending.
// An assignment >= k sets *bad (the host then reports it like lists_from_assignment's failure).  k <= 4096 (LDS: 4 k counters).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void list_hist_kernel(const uint32_t *__restrict__ assign, uint64_t n, uint32_t k, uint32_t rpb,
                                                        uint32_t nblk, uint32_t *__restrict__ cnt, uint32_t *__restrict__ bad) {
    extern __shared__ uint32_t lh_hist[];
    for (uint32_t c = threadIdx.x; c < k; c += 256) lh_hist[c] = 0u;
    __syncthreads();
    const uint64_t r0 = (uint64_t)blockIdx.x * rpb, r1 = r0 + rpb < n ? r0 + rpb : n;
    for (uint64_t r = r0 + threadIdx.x; r < r1; r += 256) {
        const uint32_t c = assign[r];
        if (c < k) atomicAdd(&lh_hist[c], 1u); else *bad = 1u;
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < k; c += 256) cnt[(uint64_t)c * nblk + blockIdx.x] = lh_hist[c];
}
__global__ __launch_bounds__(256) void list_scan_kernel(uint32_t *__restrict__ cnt, uint32_t nblk, unsigned long long *__restrict__ tot) {
    __shared__ uint32_t part[256];
    uint32_t *row = cnt + (uint64_t)blockIdx.x * nblk;
    const uint32_t per = (nblk + 255u) / 256u, b0 = threadIdx.x * per, b1 = b0 + per < nblk ? b0 + per : nblk;
    uint32_t sum = 0;
    for (uint32_t b = b0; b < b1; ++b) sum += row[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256; off <<= 1) {
        const uint32_t v = threadIdx.x >= off ? part[threadIdx.x - off] : 0u;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    uint32_t run = part[threadIdx.x] - sum;
    for (uint32_t b = b0; b < b1; ++b) { const uint32_t x = row[b]; row[b] = run; run += x; }
    if (threadIdx.x == 255) tot[blockIdx.x] = part[255];
}
__global__ __launch_bounds__(1024) void list_offsets_kernel(const unsigned long long *__restrict__ tot, uint32_t k, uint64_t n,
                                                            uint64_t *__restrict__ list_off) {
    __shared__ unsigned long long part[1024];
    const uint32_t per = (k + 1023u) / 1024u, c0 = threadIdx.x * per, c1 = c0 + per < k ? c0 + per : k;
    unsigned long long sum = 0;
    for (uint32_t c = c0; c < c1; ++c) sum += tot[c];
    part[threadIdx.x] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 1024; off <<= 1) {
        const unsigned long long v = threadIdx.x >= off ? part[threadIdx.x - off] : 0ull;
        __syncthreads();
        part[threadIdx.x] += v;
        __syncthreads();
    }
    unsigned long long run = part[threadIdx.x] - sum;
    for (uint32_t c = c0; c < c1; ++c) { list_off[c] = run; run += tot[c]; }
    if (threadIdx.x == 0) list_off[k] = n;
}
__global__ __launch_bounds__(256) void list_scatter_kernel(const uint32_t *__restrict__ assign, uint64_t n, uint32_t k, uint32_t rpb,
                                                           uint32_t nblk, const uint32_t *__restrict__ cnt,
                                                           const uint64_t *__restrict__ list_off, uint32_t *__restrict__ list_rows) {
    extern __shared__ uint32_t ls_base[];            // [4][k]: first the waves' counts, then their first slots inside the cluster
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 4u * k; i += 256) ls_base[i] = 0u;
    __syncthreads();
    const uint32_t wrows = rpb / 4u;                 // rows per wave: a multiple of 64
    const uint64_t r0 = (uint64_t)blockIdx.x * rpb + (uint64_t)wave * wrows;
    uint64_t r1 = r0 + wrows; if (r1 > n) r1 = n;
    uint32_t *mine = ls_base + (uint32_t)wave * k;
    for (uint64_t r = r0 + (uint32_t)lane; r < r1; r += 64) {
        const uint32_t c = assign[r];
        if (c < k) atomicAdd(&mine[c], 1u);
    }
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < k; c += 256) {
        uint32_t run = cnt[(uint64_t)c * nblk + blockIdx.x];       // rows of c in the blocks before this one
#pragma unroll
        for (int w = 0; w < 4; ++w) { const uint32_t x = ls_base[(uint32_t)w * k + c]; ls_base[(uint32_t)w * k + c] = run; run += x; }
    }
    __syncthreads();
    for (uint64_t rs = r0; rs < r1; rs += 64) {      // 64 rows per step, in row order
        const uint64_t r = rs + (uint32_t)lane;
        const bool valid = r < r1;
        const uint32_t c = valid ? assign[r] : 0xFFFFFFFFu;
        unsigned long long todo = __ballot(valid && c < k);
        while (todo) {
            const int l = __builtin_ctzll(todo);
            const uint32_t c0 = readlane_u32(c, l);
            const unsigned long long m = __ballot(c == c0) & todo;
            const uint32_t first = mine[c0];                                   // (wave-uniform address: a broadcast read)
            if (c == c0 && ((todo >> lane) & 1ull))
                list_rows[list_off[c0] + first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (uint32_t)r;
            wave_lds_fence();
            if (lane == l) mine[c0] = first + (uint32_t)__popcll(m);
            wave_lds_fence();
            todo &= ~m;
        }
    }
}
hipError_t launch_list_sort(const uint32_t *assign, uint64_t n, uint32_t k, uint32_t *cnt, uint32_t rows_per_block,
                            unsigned long long *tot, uint64_t *list_off, uint32_t *list_rows, uint32_t *bad, hipStream_t s) {
    if (n == 0 || k == 0 || k > 4096 || rows_per_block < 256 || (rows_per_block % 256) != 0 || n > 0xFFFFFFFFull) return hipErrorInvalidValue;
    const uint64_t nblk = (n + rows_per_block - 1) / rows_per_block;
    if (nblk > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(list_hist_kernel, dim3((uint32_t)nblk), dim3(256), (size_t)k * 4, s, assign, n, k, rows_per_block, (uint32_t)nblk, cnt, bad);
    hipLaunchKernelGGL(list_scan_kernel, dim3(k), dim3(256), 0, s, cnt, (uint32_t)nblk, tot);
    hipLaunchKernelGGL(list_offsets_kernel, dim3(1), dim3(1024), 0, s, tot, k, n, list_off);
    hipLaunchKernelGGL(list_scatter_kernel, dim3((uint32_t)nblk), dim3(256), (size_t)k * 16, s, assign, n, k, rows_per_block, (uint32_t)nblk, cnt,
                       list_off, list_rows);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// assign_kernel: Lloyd assign + final assignment (index.rs:395-424, :189-201, :244-257).
// Same skeleton as the tile re-rank: lane-per-row, 128 B of the lane's own row per step, a
// tile of CT centroids applied to it as wave-uniform scalar operands through the rolled,
// software-pipelined loop (two chunk register sets ping-ponging behind lgkmcnt(0) waits),
// running sums in LDS (lsums[centroid][lane]).  Every (row, centroid) chain is summed in
// ascending group order exactly as squared_l2_distance does; the argmin uses strict '<' in
// ascending centroid order.  Exact-order f32 VALU-bound.
// ------------------------------------------------------------------------------------
template <int CT, bool ALIGNED>
__global__ __launch_bounds__(256) void assign_kernel(const float *__restrict__ rows, uint64_t n,
                                                    uint32_t dim,
                                                    const float *__restrict__ cent, uint32_t k,
                                                    uint32_t *__restrict__ cluster,
                                                    const uint32_t *__restrict__ prev,
                                                    unsigned long long *__restrict__ changed,
                                                    unsigned long long *__restrict__ sizes) {
    __shared__ float lsums_all[4 * CT * 64];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    float *lsums = lsums_all + wave * (CT * 64);

    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = r < n;
    const float *x = rows + (valid ? r : (n - 1)) * dim;
    const uint32_t G = dim >> 2, tail = dim & 3u;
    float best = INFINITY;
    uint32_t bestc = 0;

    for (uint32_t c0 = 0; c0 < k; c0 += CT) {
        const uint32_t cnt = (k - c0 < (uint32_t)CT) ? (k - c0) : (uint32_t)CT;
        uint32_t g0 = 0;
        for (; g0 + 8 <= G; g0 += 8) {
            float4 xv[8];
#pragma unroll
            for (int g = 0; g < 8; ++g) xv[g] = load4<ALIGNED>(x + (g0 + g) * 4);
            float4 qa[8], qb[8];
            {
                const float *cp = cent + (uint64_t)c0 * dim + g0 * 4;
#pragma unroll
                for (int g = 0; g < 8; ++g) qa[g] = load4_uniform<ALIGNED>(cp + g * 4);
            }
            uint32_t cc = 0;
#pragma unroll 1
            for (; cc + 2 <= cnt; cc += 2) {
                float acc0 = g0 ? lsums[cc * 64 + lane] : 0.0f;
                float acc1 = g0 ? lsums[(cc + 1) * 64 + lane] : 0.0f;
                __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0)
                {
                    const float *cp = cent + (uint64_t)(c0 + cc + 1) * dim + g0 * 4;
#pragma unroll
                    for (int g = 0; g < 8; ++g) qb[g] = load4_uniform<ALIGNED>(cp + g * 4);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const float d0 = xv[g].x - qa[g].x, d1 = xv[g].y - qa[g].y;
                    const float d2 = xv[g].z - qa[g].z, d3 = xv[g].w - qa[g].w;
                    float t = d0 * d0 + d1 * d1;
                    t = t + d2 * d2;
                    t = t + d3 * d3;
                    acc0 = acc0 + t;
                }
                lsums[cc * 64 + lane] = acc0;
                __builtin_amdgcn_sched_barrier(0);
                __builtin_amdgcn_s_waitcnt(0xC07F);
                {
                    const uint32_t nc2 = cc + 2 < cnt ? cc + 2 : cnt - 1;
                    const float *cp = cent + (uint64_t)(c0 + nc2) * dim + g0 * 4;
#pragma unroll
                    for (int g = 0; g < 8; ++g) qa[g] = load4_uniform<ALIGNED>(cp + g * 4);
                }
                __builtin_amdgcn_sched_barrier(0);
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const float d0 = xv[g].x - qb[g].x, d1 = xv[g].y - qb[g].y;
                    const float d2 = xv[g].z - qb[g].z, d3 = xv[g].w - qb[g].w;
                    float t = d0 * d0 + d1 * d1;
                    t = t + d2 * d2;
                    t = t + d3 * d3;
                    acc1 = acc1 + t;
                }
                lsums[(cc + 1) * 64 + lane] = acc1;
                __builtin_amdgcn_sched_barrier(0);
            }
            if (cc < cnt) {
                float acc = g0 ? lsums[cc * 64 + lane] : 0.0f;
#pragma unroll
                for (int g = 0; g < 8; ++g) {
                    const float d0 = xv[g].x - qa[g].x, d1 = xv[g].y - qa[g].y;
                    const float d2 = xv[g].z - qa[g].z, d3 = xv[g].w - qa[g].w;
                    float t = d0 * d0 + d1 * d1;
                    t = t + d2 * d2;
                    t = t + d3 * d3;
                    acc = acc + t;
                }
                lsums[cc * 64 + lane] = acc;
            }
        }
        for (; g0 < G; ++g0) {
            const float4 xg = load4<ALIGNED>(x + g0 * 4);
#pragma unroll 1
            for (uint32_t cc = 0; cc < cnt; ++cc) {
                const float4 cv = load4_uniform<ALIGNED>(cent + (uint64_t)(c0 + cc) * dim + g0 * 4);
                const float d0 = xg.x - cv.x, d1 = xg.y - cv.y;
                const float d2 = xg.z - cv.z, d3 = xg.w - cv.w;
                float t = d0 * d0 + d1 * d1;
                t = t + d2 * d2;
                t = t + d3 * d3;
                const float acc = g0 ? lsums[cc * 64 + lane] : 0.0f;
                lsums[cc * 64 + lane] = acc + t;
            }
        }
        for (uint32_t e = 0; e < tail; ++e) {
            const float xe = x[G * 4 + e];
#pragma unroll 1
            for (uint32_t cc = 0; cc < cnt; ++cc) {
                const float d = xe - load1_uniform(cent + (uint64_t)(c0 + cc) * dim + G * 4 + e);
                const float acc = (G || e) ? lsums[cc * 64 + lane] : 0.0f;
                lsums[cc * 64 + lane] = acc + d * d;
            }
        }
        wave_lds_fence();
#pragma unroll 1
        for (uint32_t cc = 0; cc < cnt; ++cc) {
            const float v = lsums[cc * 64 + lane];
            if (v < best) { best = v; bestc = c0 + cc; }   // strict '<': lowest centroid wins ties
        }
        wave_lds_fence();
    }

    if (valid) cluster[r] = bestc;
    // counters: one atomic per wave and distinct cluster / per wave (every row adding to `changed` and to a
    // hundred cluster sizes on four cache lines serialises at the memory side)
    if (sizes) {
        unsigned long long m = __ballot(valid);
        while (m) {
            const uint32_t c = readlane_u32(bestc, __builtin_ctzll(m));
            const unsigned long long same = __ballot(valid && bestc == c);
            if (lane == __builtin_ctzll(m)) atomicAdd(&sizes[c], (unsigned long long)__popcll(same));
            m &= ~same;
        }
    }
    if (prev && changed) {
        const unsigned long long ch = __ballot(valid && prev[r] != bestc);
        if (lane == 0 && ch) atomicAdd(changed, (unsigned long long)__popcll(ch));
    }
}

hipError_t launch_assign(const float *rows, uint64_t n, uint32_t dim, const float *centroids,
                         uint32_t k, uint32_t *cluster, const uint32_t *prev,
                         unsigned long long *changed, unsigned long long *sizes, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (dim % 4 == 0)
        hipLaunchKernelGGL((assign_kernel<32, true>), dim3((uint32_t)blocks), dim3(256), 0, s, rows,
                           n, dim, centroids, k, cluster, prev, changed, sizes);
    else
        hipLaunchKernelGGL((assign_kernel<32, false>), dim3((uint32_t)blocks), dim3(256), 0, s, rows,
                           n, dim, centroids, k, cluster, prev, changed, sizes);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// lloyd_update: thread (c, j) adds x[r][j] over cluster c's rows in ascending r -- the
// same per-element add order as the reference's single-threaded loop (index.rs:438-444)
// -- then divides by the size (index.rs:446-453); empty clusters stay all-zero.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void lloyd_update_kernel(const float *__restrict__ rows,
                                                          uint32_t dim,
                                                          const uint32_t *__restrict__ list_rows,
                                                          const uint64_t *__restrict__ list_off,
                                                          float *__restrict__ centroids) {
    const uint32_t c = blockIdx.x;
    const uint32_t jj = blockIdx.y * 256 + threadIdx.x;
    if (jj >= dim) return;
    const uint64_t b = list_off[c], e = list_off[c + 1];
    float acc = 0.0f;
    uint64_t i = b;
    for (; i + 4 <= e; i += 4) {
        const float v0 = rows[(uint64_t)list_rows[i] * dim + jj];
        const float v1 = rows[(uint64_t)list_rows[i + 1] * dim + jj];
        const float v2 = rows[(uint64_t)list_rows[i + 2] * dim + jj];
        const float v3 = rows[(uint64_t)list_rows[i + 3] * dim + jj];
        acc = acc + v0; acc = acc + v1; acc = acc + v2; acc = acc + v3;
    }
    for (; i < e; ++i) acc = acc + rows[(uint64_t)list_rows[i] * dim + jj];
    if (e > b) acc = div_f32_ieee(acc, (float)(e - b));
    centroids[(uint64_t)c * dim + jj] = acc;
}

hipError_t launch_lloyd_update(const float *rows, uint32_t dim, const uint32_t *list_rows,
                               const uint64_t *list_off, uint32_t k, float *centroids,
                               hipStream_t s) {
    if (k == 0) return hipSuccess;
    dim3 grid(k, (dim + 255) / 256);
    hipLaunchKernelGGL(lloyd_update_kernel, grid, dim3(256), 0, s, rows, dim, list_rows, list_off,
                       centroids);
    return hipGetLastError();
}



// an empty kernel the library launches at the first call for a device (and on a new stream): the runtime loads this unit's code
// object and sets up the stream's hardware queue then, not inside the first build or the first query
__global__ void touch_build_kernel() {}
hipError_t touch_build(hipStream_t s) {
    hipLaunchKernelGGL(touch_build_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace pqv
