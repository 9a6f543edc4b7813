// kernels_half_build.hip -- the index build over a corpus of IEEE binary16 rows (pqv.h: pqv_index_build_f16 / _assign_f16 /
// _append_f16): the widening gather of the training sample, and the assignment of every row to its nearest centroid --
// assign_h_kernel (exact tier), assign_h_wide_kernel (the screen on v_mfma_f32_32x32x16_f16 with the rows AS STORED for the
// row-side operand) and assign_h_resolve_kernel (the exact chains of the rows the screen leaves undecided).
//
// The assignment of an f16 row is DEFINED as the reference's nearest_centroid (index.rs:395-424) on the row widened to f32 -- an
// exact conversion --, i.e. the 4-grouped f32 chain (index.rs:461-480) against every centroid in ascending order, strict '<' from
// +inf.  The screen only rules centroids out; what it cannot rule out is evaluated by that chain (the bound).
#include <algorithm>

#include "device_common.hpp"
#include "kernels.h"

namespace pqv {

__device__ __forceinline__ float hb_widen(uint32_t bits16) { return (float)__builtin_bit_cast(_Float16, (uint16_t)bits16); }
__device__ __forceinline__ float4 hb_widen4(uint32_t w0, uint32_t w1) {
    return make_float4(hb_widen(w0 & 0xFFFFu), hb_widen(w0 >> 16), hb_widen(w1 & 0xFFFFu), hb_widen(w1 >> 16));
}
// one term of the reference chain: the 4-group ((d0^2 + d1^2) + d2^2) + d3^2 (index.rs:466-472)
__device__ __forceinline__ float hb_group(const float4 x, const float4 c) {
    const float d0 = x.x - c.x, d1 = x.y - c.y, d2 = x.z - c.z, d3 = x.w - c.w;
    float t = d0 * d0 + d1 * d1;
    t = t + d2 * d2;
    t = t + d3 * d3;
    return t;
}

// ------------------------------------------------------------------------------------
// out[i, :] = f32(rows_h[idx ? idx[i] : i, :]): the training sample (index.rs:182-187) and, with idx == nullptr, the whole column
// where the sample is the column.  V8 (dim % 8 == 0): one 16-byte load and two 16-byte stores per thread; else element by element.
// ------------------------------------------------------------------------------------
template <bool V8>
__global__ __launch_bounds__(256) void gather_widen_h_kernel(const uint16_t *__restrict__ rows_h, const uint64_t *__restrict__ idx, uint64_t m,
                                                            uint32_t dim, float *__restrict__ out) {
    const uint32_t per_row = V8 ? dim >> 3 : dim;
    const uint64_t total = m * per_row;
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (uint64_t)gridDim.x * 256) {
        const uint64_t r = i / per_row;
        const uint32_t c = (uint32_t)(i - r * per_row);
        const uint64_t src = idx ? idx[r] : r;
        if constexpr (V8) {
            const uint4 v = *reinterpret_cast<const uint4 *>(rows_h + src * dim + c * 8);
            float4 *o = reinterpret_cast<float4 *>(out + r * dim + c * 8);
            o[0] = hb_widen4(v.x, v.y);
            o[1] = hb_widen4(v.z, v.w);
        } else {
            out[r * dim + c] = hb_widen(rows_h[src * dim + c]);
        }
    }
}
hipError_t launch_gather_widen_h(const uint16_t *rows_h, const uint64_t *idx, uint64_t m, uint32_t dim, float *out, hipStream_t s) {
    if (m == 0 || dim == 0) return hipSuccess;
    const bool v8 = (dim % 8) == 0;
    const uint64_t total = m * (v8 ? dim / 8 : dim);
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((total + 255) / 256, 16384);
    if (v8) hipLaunchKernelGGL((gather_widen_h_kernel<true>), dim3(blocks), dim3(256), 0, s, rows_h, idx, m, dim, out);
    else hipLaunchKernelGGL((gather_widen_h_kernel<false>), dim3(blocks), dim3(256), 0, s, rows_h, idx, m, dim, out);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// assign_h_kernel: the exact tier.  A lane owns a row; the block's 256 rows meet the centroids CT at a time, and a centroid tile
// passes through LDS in slices of KC dims (every lane reads the same word: an LDS broadcast).  The lane loads its row's slice in
// 5.12's load forms -- ALIGN 16 (dim % 8 == 0): eight halves per 16-byte load; 4 (even dim): two dwords per 4-group; 2: four
// ushorts -- and never reads behind the row's last element; the CT running sums stay in registers and take the 4-groups in
// ascending order, then the dim % 4 tail element by element (index.rs:474-478): the reference's chain.  Strict '<' in ascending
// centroid order from +inf: the lowest index wins a tie, NaN never wins.
// ------------------------------------------------------------------------------------
constexpr int HB_CT = 16, HB_KC = 32;
template <int ALIGN>
__global__ __launch_bounds__(256) void assign_h_kernel(const uint16_t *__restrict__ rows_h, uint64_t n, uint32_t dim, const float *__restrict__ cent,
                                                      uint32_t k, uint32_t *__restrict__ cluster) {
    constexpr int CT = HB_CT, KC = HB_KC;
    __shared__ float4 cs4[CT * KC / 4];
    float *cs = reinterpret_cast<float *>(cs4);
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool valid = r < n;
    const uint16_t *xr = rows_h + (valid ? r : 0) * dim;
    const uint32_t G = dim >> 2;
    float best = INFINITY;
    uint32_t bestc = 0;
    for (uint32_t c0 = 0; c0 < k; c0 += CT) {
        float sum[CT];
#pragma unroll
        for (int cc = 0; cc < CT; ++cc) sum[cc] = 0.0f;
        for (uint32_t d0 = 0; d0 < dim; d0 += KC) {
            __syncthreads();          // the slice before this one has been read
            for (uint32_t i = threadIdx.x; i < (uint32_t)(CT * KC); i += 256) {
                const uint32_t cc = i / KC, e = i % KC;
                cs[i] = (c0 + cc < k && d0 + e < dim) ? cent[(uint64_t)(c0 + cc) * dim + d0 + e] : 0.0f;
            }
            __syncthreads();
            if (!valid) continue;
            const uint32_t g_lo = d0 >> 2, g_hi = (G < g_lo + KC / 4) ? G : g_lo + KC / 4;
            auto apply = [&](const float4 x, uint32_t gl) {
#pragma unroll
                for (int cc = 0; cc < CT; ++cc) sum[cc] = sum[cc] + hb_group(x, cs4[cc * (KC / 4) + gl]);
            };
            if constexpr (ALIGN == 16) {          // (G is even and so is g_lo: the pairs are whole)
                for (uint32_t g = g_lo; g + 2 <= g_hi; g += 2) {
                    const uint4 v = *reinterpret_cast<const uint4 *>(xr + g * 4);
                    apply(hb_widen4(v.x, v.y), g - g_lo);
                    apply(hb_widen4(v.z, v.w), g - g_lo + 1);
                }
            } else {
                for (uint32_t g = g_lo; g < g_hi; ++g) {
                    uint32_t w0, w1;
                    if constexpr (ALIGN == 4) {
                        const uint32_t *pw = reinterpret_cast<const uint32_t *>(xr + g * 4);
                        w0 = pw[0]; w1 = pw[1];
                    } else {
                        const uint16_t *p = xr + g * 4;
                        w0 = (uint32_t)p[0] | ((uint32_t)p[1] << 16); w1 = (uint32_t)p[2] | ((uint32_t)p[3] << 16);
                    }
                    apply(hb_widen4(w0, w1), g - g_lo);
                }
            }
            // the scalar tail (elements 4 G .. dim - 1) lies in the last slice, behind every 4-group
            const uint32_t e_lo = d0 > 4 * G ? d0 : 4 * G, e_hi = dim < d0 + KC ? dim : d0 + KC;
            for (uint32_t e = e_lo; e < e_hi; ++e) {
                const float x = hb_widen(xr[e]);
#pragma unroll
                for (int cc = 0; cc < CT; ++cc) { const float d = x - cs[cc * KC + (e - d0)]; sum[cc] = sum[cc] + d * d; }
            }
        }
#pragma unroll
        for (int cc = 0; cc < CT; ++cc)
            if (c0 + cc < k && sum[cc] < best) { best = sum[cc]; bestc = c0 + cc; }
    }
    if (valid) cluster[r] = bestc;
}
hipError_t launch_assign_h(const uint16_t *rows_h, uint64_t n, uint32_t dim, const float *centroids, uint32_t k, uint32_t *cluster, hipStream_t s) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255) / 256;
    if (blocks > 0x7FFFFFFFull || dim == 0) return hipErrorInvalidValue;
    if (dim % 8 == 0) hipLaunchKernelGGL((assign_h_kernel<16>), dim3((uint32_t)blocks), dim3(256), 0, s, rows_h, n, dim, centroids, k, cluster);
    else if (dim % 2 == 0) hipLaunchKernelGGL((assign_h_kernel<4>), dim3((uint32_t)blocks), dim3(256), 0, s, rows_h, n, dim, centroids, k, cluster);
    else hipLaunchKernelGGL((assign_h_kernel<2>), dim3((uint32_t)blocks), dim3(256), 0, s, rows_h, n, dim, centroids, k, cluster);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// bias[s] = |c - mu|^2 + 2 mu.(c - mu) of the centroid in sorted slot s (c = centroids[perm[s]]), summed in f64 and rounded once;
// +inf in the padding slots [kc, kc_pad): their scores never win and never become candidates.  One wave per slot.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_bias_kernel(const float *__restrict__ cent, const float *__restrict__ mu, const uint32_t *__restrict__ perm,
                                                       uint32_t kc, uint32_t kc_pad, uint32_t dim, float *__restrict__ bias) {
    const int lane = threadIdx.x & 63;
    const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (s >= kc_pad) return;
    if (s >= kc) { if (lane == 0) bias[s] = INFINITY; return; }
    const float *c = cent + (uint64_t)perm[s] * dim;
    double acc = 0.0;
    for (uint32_t e = lane; e < dim; e += 64) {
        const double m = (double)mu[e], cc = (double)c[e] - m;
        acc += cc * cc + 2.0 * m * cc;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __builtin_bit_cast(double, shfl_u64(__builtin_bit_cast(uint64_t, acc), lane ^ off));
    if (lane == 0) bias[s] = (float)acc;
}
hipError_t launch_half_bias(const float *centroids, const float *mu, const uint32_t *perm, uint32_t kc, uint32_t kc_pad, uint32_t dim, float *bias,
                            hipStream_t s) {
    if (kc_pad == 0) return hipSuccess;
    hipLaunchKernelGGL(half_bias_kernel, dim3((kc_pad + 3) / 4), dim3(256), 0, s, centroids, mu, perm, kc, kc_pad, dim, bias);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// assign_h_wide_kernel (kernels.h: AssignHalfArgs).  |x - c|^2 = |x - mu|^2 + s_c,  s_c = b_c - 2 x.(c - mu): the first term is
// the row's own, so the argmin over c is the argmin of the score s_c, and its contraction takes the row AS STORED.
//
// Block = 256 rows against all centroids, 256 at a time; 8 waves as 2 (centroid side, M) x 4 (row side, N), each 128 centroids x
// 64 rows = 4 x 2 tiles of v_mfma_f32_32x32x16_f16; K in 128-byte stages through double-buffered, chunk-swizzled LDS
// (assign_wide_kernel's loop).  C/D layout: col = lane & 31 is a DATA ROW, so a lane owns two rows and a row's running best needs
// no cross-lane reduction.
//   row side   the rows are 2 dim bytes apart, unpadded: a thread stages the 16-byte chunks (row ld_r + 64 h, chunk ld_ch of the
//              stage) through a buffer descriptor that ends at the LAST BYTE of the call's rows (beyond it the load returns zero
//              and touches nothing); a chunk at or beyond the row's own end lies in the NEXT row and is replaced by zeros before
//              it reaches LDS (its bytes could be Inf / NaN: NaN x 0 = NaN).
//   |x|^2      from the row operands a lane reads for the matrix instruction anyway, during the first centroid tile: lane (l31, lk)
//              holds the chunks 2 j + lk of its two rows, four v_dot2 per chunk, one cross-half shuffle at the end.  A non-finite
//              sum <=> a non-finite element: the call's flag.
//   t_c        = fma(-kA, acc, b_c), kA = 2 / cscale;  |t_c - s_c| <= E = xs grp_a + grp_b per 32-centroid group (xs >= |x|)
//   best       = min_c (t_c + E) over all centroids: per lane, one cross-half shuffle, one LDS atomicMin per wave pair
//   keep c    <=> !(t_c - E > cut(best)): every centroid whose reference distance could be <= that of the best one
// ------------------------------------------------------------------------------------
// U = pub + ub_best >= |x - mu|^2 + s_* = the distance to the centroid of the smallest upper-bound score; a centroid c can reach a
// reference distance <= that one's only if d_c (1 - cm) <= d_* (1 + cm), i.e. s_c <= ub_best + U 2 cm / (1 - cm)
__device__ __forceinline__ float hb_cut(float pub, float ub_best, float cm) {
    const float U = fmaxf(pub + ub_best, 0.0f) * 1.000001f + 1.0e-30f;
    const float slack = U * (2.0f * cm / (1.0f - cm)) * 1.000001f;
    return ub_best + slack + 4.0e-7f * (fabsf(ub_best) + slack) + 1.0e-30f;          // the f32 roundings of this expression, upward
}
// xs >= |x| and pub >= |x - mu|^2 from the kernel's own f32 sum of squares (xn_up: its summation margin; xn_add: the squares of
// subnormal halves, should the dot instruction flush them)
__device__ __forceinline__ void hb_row_bounds(float sumsq, float xn_up, float xn_add, float mun, float &xs, float &pub) {
    xs = sqrtf(sumsq * xn_up + xn_add) * 1.000001f;
    const float p = xs + mun;
    pub = p * p * 1.000001f;
}

typedef _Float16 hb_half2 __attribute__((ext_vector_type(2)));
struct hb_h2x4 { hb_half2 p[4]; };
constexpr int HW_TM = 4, HW_TN = 2, HW_NWM = 2, HW_NWN = 4, HW_ST = 8;
constexpr int HW_BM = 32 * HW_TM * HW_NWM, HW_BN = 32 * HW_TN * HW_NWN, HW_NT = 64 * HW_NWM * HW_NWN;     // 256 centroids x 256 rows, 512 threads
__global__ __launch_bounds__(HW_NT, 1) void assign_h_wide_kernel(const AssignHalfArgs a) {
    constexpr int TM = HW_TM, TN = HW_TN, BM = HW_BM, BN = HW_BN, NT = HW_NT, ST = HW_ST, NWN = HW_NWN;
    constexpr int CA = BM * ST / NT, CB = BN * ST / NT;        // 16-byte chunks a thread stages per K stage and side
    extern __shared__ float4 hw_lds[];                         // [2][BM * ST] centroid stages, [2][BN * ST] row stages
    float4 *const As4 = hw_lds, *const Bs4 = hw_lds + 2 * BM * ST;
    auto sw = [](int r) { return ((r >> 1) & 1) | (((r >> 2) & 3) << 1); };      // 128-byte rows: assign_wide_kernel's swizzle
    __shared__ float bc_s[BM];               // bias of the current centroid tile (+inf beyond kc)
    __shared__ float ga_s[BM / 32], gb_s[BM / 32];       // per 32-centroid group of the tile: E = xs ga + gb
    __shared__ float xn_s[BN];               // the rows' sums of squares
    __shared__ uint32_t best_s[BN];          // sortable bits of the rows' smallest upper-bound score so far

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave / NWN, wn = wave % NWN;
    const uint64_t n0 = (uint64_t)blockIdx.x * BN;             // first data row of the block
    const uint32_t xbytes = a.dim * 2, cbytes = a.dim_p * 2;
    constexpr int RPS = NT / ST;
    const int ld_r = tid / ST, ld_ch = tid % ST;
    float4 ra[CA], rb[CB];
    uint32_t rb_kb = 0;                                        // the K offset of the row chunks in rb
    const uint64_t vleft = (a.m - n0) * xbytes;
    const __amdgpu_buffer_rsrc_t vres = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint16_t *>(a.rows_h + n0 * a.dim), 0, (int)(vleft > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)vleft), 0x00020000);
    const uint32_t lane_x = (uint32_t)ld_r * xbytes + (uint32_t)ld_ch * 16, step_x = (uint32_t)RPS * xbytes;
    const uint32_t lane_c = (uint32_t)ld_r * cbytes + (uint32_t)ld_ch * 16, step_c = (uint32_t)RPS * cbytes;
    if (tid < BN) best_s[tid] = 0xFFFFFFFFu;

    const int l31 = lane & 31, lk = lane >> 5;
    int rowa[TM], rowb[TN], swa[TM], swb[TN];
#pragma unroll
    for (int t = 0; t < TM; ++t) { rowa[t] = wm * 32 * TM + t * 32 + l31; swa[t] = sw(rowa[t]); }
#pragma unroll
    for (int t = 0; t < TN; ++t) { rowb[t] = wn * 32 * TN + t * 32 + l31; swb[t] = sw(rowb[t]); }
    uint64_t grow[TN];
#pragma unroll
    for (int j = 0; j < TN; ++j) grow[j] = n0 + (uint64_t)rowb[j];
    float xsq[TN];                                             // the lane's share of its rows' sums of squares (first centroid tile)
#pragma unroll
    for (int j = 0; j < TN; ++j) xsq[j] = 0.0f;
    const uint32_t nk = cbytes / (16 * ST);

    for (uint32_t c0 = 0; c0 < a.kc; c0 += BM) {
        const bool first = c0 == 0;
        const uint64_t qleft = (uint64_t)(a.kc_pad - c0) * cbytes;
        const __amdgpu_buffer_rsrc_t qres = __builtin_amdgcn_make_buffer_rsrc(
            const_cast<uint16_t *>(a.c16 + (uint64_t)c0 * a.dim_p), 0, (int)(qleft > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t)qleft), 0x00020000);
        auto fetch = [&](uint32_t kb) {
#pragma unroll
            for (int h = 0; h < CA; ++h) ra[h] = buf_ld16(qres, lane_c, kb + h * step_c);
#pragma unroll
            for (int h = 0; h < CB; ++h) rb[h] = buf_ld16(vres, lane_x, kb + h * step_x);
            rb_kb = kb;
        };
        auto stash = [&](int buf) {
            const bool rb_own = rb_kb + (uint32_t)ld_ch * 16 < xbytes;          // else the chunks lie in the NEXT rows
#pragma unroll
            for (int h = 0; h < CA; ++h) { const int r = ld_r + RPS * h; As4[buf * BM * ST + r * ST + (ld_ch ^ sw(r))] = ra[h]; }
#pragma unroll
            for (int h = 0; h < CB; ++h) {
                const int r = ld_r + RPS * h;
                const float4 v = rb_own ? rb[h] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                Bs4[buf * BN * ST + r * ST + (ld_ch ^ sw(r))] = v;
            }
        };
        if (tid < BM) bc_s[tid] = a.bias[c0 + tid];
        if (tid < BM / 32) { ga_s[tid] = a.grp_a[c0 / 32 + tid]; gb_s[tid] = a.grp_b[c0 / 32 + tid]; }
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
                if (first) {
#pragma unroll
                    for (int jj = 0; jj < TN; ++jj) {
                        const hb_h2x4 hv = __builtin_bit_cast(hb_h2x4, bv[set][jj]);
#pragma unroll
                        for (int e = 0; e < 4; ++e) xsq[jj] = __builtin_amdgcn_fdot2(hv.p[e], hv.p[e], xsq[jj], false);
                    }
                }
            }
            if (kt + 1 < nk) stash(buf ^ 1);
            __syncthreads();
        }
        if (first) {
            // the rows' sums of squares: lane (l31, lk) has read the chunks 2 j + lk of its rows, the other half-wave the rest
#pragma unroll
            for (int j = 0; j < TN; ++j) {
                const float s = xsq[j] + __shfl_xor(xsq[j], 32, 64);
                if (wm == 0 && lk == 0) {
                    xn_s[rowb[j]] = s;
                    if (grow[j] < a.m && !(s <= 3.0e38f)) atomicOr(a.flag, 1u);      // Inf / NaN in the row: the call steps down
                }
            }
            __syncthreads();
        }
        float xs[TN], pub[TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) hb_row_bounds(xn_s[rowb[j]], a.xn_up, a.xn_add, a.mun, xs[j], pub[j]);
        // ---- pass 1: t in place of the accumulators; per 32-centroid group the error term E (the centroids are sorted by norm:
        // a group's own maxima scale its bound), the lane's smallest upper- and lower-bound scores per row
        float mub[TN], mlb[TN], Eg[TM][TN];
#pragma unroll
        for (int j = 0; j < TN; ++j) { mub[j] = INFINITY; mlb[j] = INFINITY; }
#pragma unroll
        for (int i = 0; i < TM; ++i) {
            const float ga = ga_s[wm * TM + i], gb = gb_s[wm * TM + i];
            float mt[TN];
#pragma unroll
            for (int j = 0; j < TN; ++j) { Eg[i][j] = __builtin_fmaf(xs[j], ga, gb) * 1.000001f; mt[j] = INFINITY; }
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const float bc = bc_s[wm * 32 * TM + i * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk];
#pragma unroll
                for (int j = 0; j < TN; ++j) {
                    const float t = __builtin_fmaf(-a.kA, acc[i][j][r], bc);
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
            const float cut = hb_cut(pub[j], bb == 0xFFFFFFFFu ? INFINITY : unsortable_bits(bb), a.cm);
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
        __syncthreads();          // bc_s, the group tables and the LDS stages are rewritten by the next centroid tile
    }
    if (tid < BN && n0 + tid < a.m) {
        const uint32_t bb = best_s[tid];
        a.best_t[n0 + tid] = bb == 0xFFFFFFFFu ? INFINITY : unsortable_bits(bb);
        float x1, p1;
        hb_row_bounds(xn_s[tid], a.xn_up, a.xn_add, a.mun, x1, p1);
        a.pub[n0 + tid] = p1;
    }
}
hipError_t launch_assign_h_wide(const AssignHalfArgs &a, hipStream_t s) {
    if (a.m == 0 || a.kc == 0) return hipSuccess;
    if ((a.dim % 8) != 0 || a.dim == 0 || a.dim_p != (a.dim + 63) / 64 * 64 || (uint64_t)a.dim_p * 2 * 512 >= 0x7FFFFFFFull ||
        (a.kc_pad % HW_BM) != 0 || a.kc_pad < a.kc || a.cap == 0)
        return hipErrorInvalidValue;
    const uint64_t blocks = (a.m + HW_BN - 1) / HW_BN;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    constexpr size_t lds = 2 * (size_t)(HW_BM + HW_BN) * HW_ST * 16;
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(assign_h_wide_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    hipLaunchKernelGGL(assign_h_wide_kernel, dim3((uint32_t)blocks), dim3(HW_NT), lds, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// assign_h_resolve_kernel: assign_resolve_kernel over 2-byte rows.  A wave owns 16 rows x 4 candidate slots per round.  A row's
// candidates are first filtered against the row's FINAL best; a row left with one survivor is done -- its row is never read --
// and only rows with two or more (or an overflowed list: every centroid) go through the exact chains on the widened row: lane g
// forms the 4-group term of group g (one 8-byte load of the row), lane `slot` adds its pair's terms in ascending group order.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void assign_h_resolve_kernel(const AssignHalfArgs a, const float *__restrict__ centroids, uint32_t *__restrict__ cluster,
                                                              unsigned long long *__restrict__ stats) {
    __shared__ float lds_all[2][64 * 65];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    float *lds = lds_all[wv];
    const uint32_t dim = a.dim;
    const uint64_t wave_row0 = ((uint64_t)blockIdx.x * 2 + (uint32_t)wv) * 16;
    const uint64_t row = wave_row0 + (uint32_t)(lane >> 2);
    const uint32_t cl = (uint32_t)lane & 3u;
    const bool live = row < a.m;
    uint32_t cnt = live ? a.cand_cnt[row] : 0u;
    const bool all = cnt > a.cap;                     // list overflowed: every centroid is a candidate
    float cut = INFINITY;
    if (live && !all) cut = hb_cut(a.pub[row], a.best_t[row], a.cm);
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
                const uint32_t m4 = (uint32_t)(mask >> (4 * r)) & 0xFu;     // wave-uniform (a set bit: the row exists)
                if (m4 == 0) continue;
                const uint2 xw = *reinterpret_cast<const uint2 *>(a.rows_h + (wave_row0 + (uint32_t)r) * dim + goff);
                const float4 xv = hb_widen4(xw.x, xw.y);
                float4 cv[4];
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const uint32_t jp = readlane_u32(j, 4 * r + u);
                    cv[u] = load4<true>(centroids + (uint64_t)jp * dim + goff);
                }
#pragma unroll
                for (int u = 0; u < 4; ++u) {
                    const float tt = hb_group(xv, cv[u]);
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
hipError_t launch_assign_h_resolve(const AssignHalfArgs &a, const float *centroids, uint32_t *cluster, unsigned long long *stats, hipStream_t s) {
    if (a.m == 0) return hipSuccess;
    if ((a.dim % 8) != 0) return hipErrorInvalidValue;
    const uint64_t wblocks = (a.m + 31) / 32;
    if (wblocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(assign_h_resolve_kernel, dim3((uint32_t)wblocks), dim3(128), 0, s, a, centroids, cluster, stats);
    return hipGetLastError();
}

}  // namespace pqv
