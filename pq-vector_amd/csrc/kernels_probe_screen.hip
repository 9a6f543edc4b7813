// kernels_probe_screen.hip -- the screened centroid probe of a batch (kernels.h: ProbeScreenArgs): probe_screen_kernel, an f16
// contraction of the batch's query images against the centroid images on the matrix cores, and probe_resolve_kernel, which
// turns every score into rigorous bounds of the REFERENCE distance (src/ivf/index.rs:461-480), keeps the centroids that can be
// among a query's P nearest and evaluates only those in probe_rows_kernel's arithmetic and order.  Output: probe_rows_kernel's
// partial lists with KEY_EMPTY in place of every centroid the bounds exclude -- the probe merge is the same launch as before.
#include "device_common.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// probe_screen_kernel: score[q][c] = image(q) . image(c), f32 accumulation.
//
// grid = (kc_pad / 64, ceil(nq / 64)); a block owns a 64 x 64 tile, 2 x 2 tiles of v_mfma_f32_32x32x16_f16, and its 4 waves
// split K: wave w takes the 128-byte K stages w, w + 4, ... of the WHOLE tile and the four partial tiles meet in LDS at the end
// (the bound allows the accumulation any order).  A wave stages its operands itself: sixteen coalesced 16-byte loads per stage
// (8 lanes cover one row's 128 bytes, 8 rows per instruction), parked in its own 16 KB of LDS at assign_wide_kernel's chunk
// swizzle, read back as MFMA fragments -- no block barrier inside the K loop.  The operands come from L2 (C3: 1.5 MB of centroid images, 1.5 MB of query images), 50 MB in
// all; with 32 x 32 tiles whose lanes fetched their fragments straight from the row-major images (32 lines touched per
// instruction, 100 MB) the kernel ran 15 us.
// C layout: column = lane & 31 is the centroid (coalesced stores), the 16 registers are queries (r & 3) + 8 (r >> 2) + 4 (lane >> 5).
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256, 2) void probe_screen_kernel(const ProbeScreenArgs a) {
    if (a.zero_u32 && blockIdx.x == 0) {     // scratch the NEXT kernels expect zeroed (as probe_rows_kernel)
        for (uint32_t i = blockIdx.y * 256 + threadIdx.x; i < a.zero_n; i += gridDim.y * 256) a.zero_u32[i] = 0u;
    }
    __shared__ float4 lds[4096];             // per wave: [64 rows][8 chunks] query stage, the same of centroids; then the partial tiles
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);      // (the K loop is wave-uniform)
    const int l31 = lane & 31, lk = lane >> 5;
    float4 *const As = lds + wave * 1024, *const Bs = As + 512;
    auto sw = [](int r) { return ((r >> 1) & 1) | (((r >> 2) & 3) << 1); };
    const uint32_t q0 = blockIdx.y * 64u, c0 = blockIdx.x * 64u;                // c0 + 63 < kc_pad (a multiple of 256)
    const int ld_r = lane >> 3, ld_ch = lane & 7;
    const uint32_t rowb = a.dim_p / 8u;                                        // float4 per image row
    const float4 *const qb = reinterpret_cast<const float4 *>(a.q16) + (uint64_t)q0 * rowb + ld_ch;
    const float4 *const cb = reinterpret_cast<const float4 *>(a.c16) + (uint64_t)(c0 + ld_r) * rowb + ld_ch;
    uint32_t qo[8];                          // float4 offset of the lane's h-th query row from the tile's first
#pragma unroll
    for (int h = 0; h < 8; ++h) {
        const uint32_t qr = q0 + ld_r + 8 * h < a.nq ? q0 + ld_r + 8 * h : a.nq - 1;      // (rows beyond the batch: clamped, never stored)
        qo[h] = (qr - q0) * rowb;
    }
    const uint32_t nk = a.dim_p / 64u;                                         // 128-byte stages
    f32x16_t acc00, acc01, acc10, acc11;     // (query half, centroid half)
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc00[r] = 0.0f; acc01[r] = 0.0f; acc10[r] = 0.0f; acc11[r] = 0.0f; }
    for (uint32_t kt = wave; kt < nk; kt += 4) {
        float4 ra[8], rb[8];                 // (sixteen loads in flight; the block's other waves and the CU's other block cover the wait)
#pragma unroll
        for (int h = 0; h < 8; ++h) { ra[h] = qb[qo[h] + kt * 8]; rb[h] = cb[(uint32_t)(8 * h) * rowb + kt * 8]; }
#pragma unroll
        for (int h = 0; h < 8; ++h) {
            const int r = ld_r + 8 * h;
            As[r * 8 + (ld_ch ^ sw(r))] = ra[h];
            Bs[r * 8 + (ld_ch ^ sw(r))] = rb[h];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            float4 av[2], bv[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int r = t * 32 + l31;
                av[t] = As[r * 8 + ((2 * j + lk) ^ sw(r))];
                bv[t] = Bs[r * 8 + ((2 * j + lk) ^ sw(r))];
            }
            acc00 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, av[0]), __builtin_bit_cast(f16x8_t, bv[0]), acc00, 0, 0, 0);
            acc01 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, av[0]), __builtin_bit_cast(f16x8_t, bv[1]), acc01, 0, 0, 0);
            acc10 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, av[1]), __builtin_bit_cast(f16x8_t, bv[0]), acc10, 0, 0, 0);
            acc11 = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, av[1]), __builtin_bit_cast(f16x8_t, bv[1]), acc11, 0, 0, 0);
        }
    }
    // the four partial tiles: wave w leaves its 64 registers in its own 16 KB, then adds and stores tile (w >> 1, w & 1)
    __syncthreads();
    float *red = reinterpret_cast<float *>(lds);
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        red[((wave * 4 + 0) * 16 + r) * 64 + lane] = acc00[r];
        red[((wave * 4 + 1) * 16 + r) * 64 + lane] = acc01[r];
        red[((wave * 4 + 2) * 16 + r) * 64 + lane] = acc10[r];
        red[((wave * 4 + 3) * 16 + r) * 64 + lane] = acc11[r];
    }
    __syncthreads();
    const int tm = wave >> 1, tn = wave & 1;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
        const int o = ((tm * 2 + tn) * 16 + r) * 64 + lane;
        const float v = (red[o] + red[4096 + o]) + (red[8192 + o] + red[12288 + o]);
        const uint32_t q = q0 + (uint32_t)(tm * 32 + (r & 3) + 8 * (r >> 2) + 4 * lk);
        if (q < a.nq) a.score[(uint64_t)q * a.kc_pad + c0 + (uint32_t)(tn * 32 + l31)] = v;
    }
}

// ------------------------------------------------------------------------------------
// The bound.  With a = fl(q - mu), b = fl(c - mu) (f32 vectors), an2 / bn2 their norms as
// center_normalize_f16_kernel summed them and s the score:
//   est = s (sqrt(an2) / 2^8) / cscale                                  ~ a . b
//   mid = (an2 + bn2) - 2 est                                           ~ |a - b|^2
//   E   = kS (an2 + bn2) + 2 |a| (|b| e1 + e2 / cscale) + tiny          >= | |q - c|^2 - mid |
//   (mid - E)(1 - cm) <= d_ref(q, c) <= (mid + E)(1 + cm)
// e1: f16 rounding of both images (2 h + h^2), f32 accumulation of the contraction in any order, the roundings of est;
// e2: what f16 subnormals cost a centroid image whose components fall below 2^-14 at the table-wide scale; kS: the norms' own
// summation error, the roundings of (q - mu) and (c - mu) and of the expression; cm: the reference chain's own rounding.
// ------------------------------------------------------------------------------------
struct ProbeBound { float lb, ub; };
__device__ __forceinline__ ProbeBound probe_bound(const ProbeScreenArgs &a, float an2, float an_ub, float bn2, float s) {
    const float bn_ub = sqrtf(bn2) * a.fn;
    const float est = s * (sqrtf(an2) * 0.00390625f) * a.inv_cs;
    const float S = an2 + bn2;
    const float mid = S - 2.0f * est;
    const float E = (a.kS * S + 2.0f * an_ub * (bn_ub * a.e1 + a.e2s)) * 1.00001f + 1.0e-33f;
    ProbeBound r;
    // An intermediate that overflowed says nothing about the pair: fmaxf(NaN, 0) is 0, so inf - inf in `mid` would come out as a
    // tiny UPPER bound.  Every value the bounds are made of must be finite, else the pair is unbounded (lb 0, ub +inf: it stays a
    // contender and can never define the threshold).  The same holds for an upper bound so close to FLT_MAX that the reference
    // chain, which rounds upwards too, may have overflowed to +inf where the bound stays finite.
    const float lo = mid - E, hi = mid + E;
    const bool finite = fabsf(S) < INFINITY && fabsf(est) < INFINITY && fabsf(mid) < INFINITY && E < INFINITY &&
                        fabsf(lo) < INFINITY && hi < 3.0e38f;      // (below 3e38 (1 + cm) the reference chain itself cannot overflow)
    r.lb = finite ? fmaxf(lo, 0.0f) * a.lo_f : 0.0f;
    r.ub = finite ? fmaxf(hi, 0.0f) * a.hi_f + 1.0e-33f : INFINITY;
    return r;
}

constexpr uint32_t PR_CAP = 2048;        // contenders a query may keep before it goes all-exact
constexpr uint32_t PR_GS = 192;          // float4 groups of a row per slab of terms (three per lane)
constexpr uint32_t PR_TW = PR_GS + 4;    // words per contender in the slab (the summing lanes' 16-byte reads fall on different banks)
constexpr uint32_t PR_R = 32;            // contenders per round: 8 per wave

// ------------------------------------------------------------------------------------
// probe_resolve_kernel: one block of 256 threads per query.
//   1. T = the np-th smallest UPPER bound (block_kth_u32 over the bounds parked in LDS): np centroids have a reference distance <= T
//   2. contenders = centroids whose LOWER bound is <= T ('<=': every tie at the np-th place stays); the others are written
//      KEY_EMPTY right away
//   3. the contenders' exact distances, 8 per wave and round.  The reference's arithmetic splits into per-group terms
//      ((d0^2 + d1^2) + d2^2) + d3^2, which are independent, and ONE running sum over them, which is a chain.  The terms are
//      made by all 64 lanes -- lane l takes groups l, l + 64, l + 128 of a slab of every contender: coalesced row reads, twelve
//      loads in flight, the query's groups in registers -- and parked in LDS; lane i < 8 then adds contender i's terms in order.
//      (Handing the sum through 8 lanes per contender, resolve_exact's scheme, left the kernel a chain of L2 round trips and
//      shuffles: 35 us on C3.)
// A query whose norm or threshold is not finite, or that keeps more than PR_CAP contenders, evaluates EVERY centroid.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void probe_resolve_kernel(const ProbeScreenArgs a) {
    __shared__ uint32_t s_hist[256];
    __shared__ uint32_t s_sel[4];
    __shared__ uint32_t s_list[PR_CAP];
    __shared__ __attribute__((aligned(16))) float s_term[PR_R * PR_TW];
    const uint32_t q = blockIdx.x;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float an2 = a.qn2[q];
    const float an_ub = sqrtf(an2) * a.fn;
    const float *sc = a.score + (uint64_t)q * a.kc_pad;
    uint64_t *pk = a.part_keys + (uint64_t)q * a.kc_pad;
    uint32_t *pv = a.part_vals + (uint64_t)q * a.kc_pad;
    bool all = !(an2 < INFINITY);               // (NaN included)
    float Tf = INFINITY;
    // both bounds of every centroid parked in LDS (the slab of terms is not in use yet) where they fit; else made again per read
    const bool parked = 2u * a.kc <= PR_R * PR_TW;
    float *s_ub = s_term, *s_lb = s_term + a.kc;
    auto bound = [&](uint32_t c) {
        ProbeBound b = probe_bound(a, an2, an_ub, a.cn2[c], sc[c]);
        if (!(b.ub < INFINITY)) b.ub = INFINITY;            // (NaN counts as +inf)
        return b;
    };
    auto ub_of = [&](uint32_t c) { return parked ? s_ub[c] : bound(c).ub; };
    if (!all) {
        // The upper bounds of one query share their leading bits (C3: all within a few per cent of each other), and a radix
        // select over the raw bits would send a whole pass into one histogram bin.  So the select runs on keys spread over 32
        // bits, key = (ub - min) / (max - min) scaled: non-decreasing in ub, and the threshold is then the LARGEST upper bound
        // whose key does not exceed the np-th smallest key -- at least np centroids lie at or below it, which is all the
        // argument needs (where two bounds share a key the threshold may sit a hair above the np-th smallest bound).
        if (threadIdx.x == 0) { s_sel[2] = 0x7F800000u; s_sel[3] = 0u; }
        __syncthreads();
        uint32_t mn = 0x7F800000u, mx = 0u;
        for (uint32_t c = threadIdx.x; c < a.kc; c += 256) {
            const ProbeBound b = bound(c);
            if (parked) { s_ub[c] = b.ub; s_lb[c] = b.lb; }
            if (b.ub < INFINITY) { const uint32_t u = __float_as_uint(b.ub); mn = u < mn ? u : mn; mx = u > mx ? u : mx; }     // (ub >= 0: bits order like values)
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const uint32_t on = (uint32_t)__shfl_xor((int)mn, off, 64), ox = (uint32_t)__shfl_xor((int)mx, off, 64);
            mn = on < mn ? on : mn; mx = ox > mx ? ox : mx;
        }
        if (lane == 0) { atomicMin(&s_sel[2], mn); atomicMax(&s_sel[3], mx); }
        __syncthreads();
        const float fmn = __uint_as_float(s_sel[2]), fmx = __uint_as_float(s_sel[3]);
        const float scale = fmx > fmn ? 4.0e9f / (fmx - fmn) : 0.0f;
        auto key_of = [&](uint32_t c) {
            const float ub = ub_of(c);
            if (!(ub < INFINITY)) return 0xFFFFFFFFu;
            // in [0, 4e9 (1 + 2^-22)] < 2^32 -- unless the bounds spread by less than ~1e-29 (all distances ~ 0): scale is then
            // +inf, the smallest bound's key 0 * inf = NaN and the others' +inf, all of which land on 0xFFFFFFFE: one key for
            // every centroid, so the threshold is the largest upper bound (conservative)
            const float kf = (ub - fmn) * scale;
            return kf < 4.2e9f ? (uint32_t)kf : 0xFFFFFFFEu;
        };
        __syncthreads();                                    // (s_sel is block_kth_u32's scratch from here on)
        const uint32_t Tk = block_kth_u32(key_of, a.kc, a.np, s_hist, s_sel);
        if (threadIdx.x == 0) s_sel[3] = Tk == 0xFFFFFFFFu ? 0x7F800000u : 0u;
        __syncthreads();
        if (Tk != 0xFFFFFFFFu) {
            uint32_t tm = 0u;
            for (uint32_t c = threadIdx.x; c < a.kc; c += 256)
                if (key_of(c) <= Tk) { const uint32_t u = __float_as_uint(ub_of(c)); tm = u > tm ? u : tm; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) { const uint32_t o = (uint32_t)__shfl_xor((int)tm, off, 64); tm = o > tm ? o : tm; }
            if (lane == 0) atomicMax(&s_sel[3], tm);
        }
        __syncthreads();
        Tf = __uint_as_float(s_sel[3]);
        all = !(Tf < INFINITY);
    }
    __syncthreads();
    if (threadIdx.x == 0) s_sel[2] = 0u;
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < a.kc_pad; c += 256) {
        bool keep = false;
        if (c < a.kc && !all) {
            const float lb = parked ? s_lb[c] : bound(c).lb;
            keep = !(lb > Tf);
        }
        if (keep) {
            const uint32_t slot = atomicAdd(&s_sel[2], 1u);
            if (slot < PR_CAP) s_list[slot] = c;
        } else {
            pk[c] = KEY_EMPTY; pv[c] = 0xFFFFFFFFu;
        }
    }
    __syncthreads();
    uint32_t m = s_sel[2];
    if (all || m > PR_CAP) { all = true; m = a.kc; }
    if (a.stats && threadIdx.x == 0) {
        atomicAdd(&a.stats[0], 1ull);
        atomicAdd(&a.stats[1], (unsigned long long)m);
        if (all) atomicAdd(&a.stats[2], 1ull);
    }
    // exact chains: probe_rows_kernel's  t = ((d0^2 + d1^2) + d2^2) + d3^2;  sum = sum + t  per float4, in order, no FMA
    const uint32_t G = a.dim >> 2;
    const float4 *qg = reinterpret_cast<const float4 *>(a.queries + (uint64_t)q * a.dim);
    for (uint32_t p0 = 0; p0 < m; p0 += PR_R) {
        // contender p0 + 4 i + wave is the wave's i-th of the round (a short last round spreads over the four waves)
        float run = 0.0f;                                    // lane i < 8: the wave's i-th
        for (uint32_t gs0 = 0; gs0 < G; gs0 += PR_GS) {
            float4 qv[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const uint32_t g = gs0 + (uint32_t)lane + 64u * (uint32_t)j;
                qv[j] = qg[g < G ? g : G - 1];
            }
#pragma unroll
            for (int half = 0; half < 2; ++half) {
                float4 xv[4][3];
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const uint32_t pi = p0 + 4u * (uint32_t)(half * 4 + i) + (uint32_t)wave;
                    if (pi < m) {                                             // (wave-uniform)
                        const uint32_t c = all ? pi : s_list[pi];
                        const float4 *xg = reinterpret_cast<const float4 *>(a.centroids + (uint64_t)c * a.dim);
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            const uint32_t g = gs0 + (uint32_t)lane + 64u * (uint32_t)j;
                            xv[i][j] = xg[g < G ? g : G - 1];
                        }
                    } else {
#pragma unroll
                        for (int j = 0; j < 3; ++j) xv[i][j] = make_float4(0.f, 0.f, 0.f, 0.f);       // never summed
                    }
                }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 3; ++j) {
                        const float d0 = qv[j].x - xv[i][j].x, d1 = qv[j].y - xv[i][j].y, d2 = qv[j].z - xv[i][j].z, d3 = qv[j].w - xv[i][j].w;
                        float t = d0 * d0 + d1 * d1;
                        t = t + d2 * d2;
                        t = t + d3 * d3;
                        s_term[((uint32_t)wave * 8u + (uint32_t)(half * 4 + i)) * PR_TW + (uint32_t)lane + 64u * (uint32_t)j] = t;
                    }
            }
            __syncthreads();
            if (lane < 8) {
                const uint32_t n = G - gs0 < PR_GS ? G - gs0 : PR_GS;
                const float *row = s_term + ((uint32_t)wave * 8u + (uint32_t)lane) * PR_TW;
                uint32_t g = 0;
#pragma unroll 4
                for (; g + 4 <= n; g += 4) {
                    const float4 t = *reinterpret_cast<const float4 *>(row + g);
                    run = run + t.x; run = run + t.y; run = run + t.z; run = run + t.w;
                }
                for (; g < n; ++g) run = run + row[g];
            }
            __syncthreads();
        }
        if (lane < 8 && p0 + 4u * (uint32_t)lane + (uint32_t)wave < m) {
            const uint32_t li = p0 + 4u * (uint32_t)lane + (uint32_t)wave;
            const uint32_t c = all ? li : s_list[li];
            pk[c] = ((uint64_t)__float_as_uint(run) << 32) | c;
            pv[c] = c;
        }
    }
}

hipError_t launch_probe_screen(const ProbeScreenArgs &a, hipStream_t s) {
    if (a.nq == 0 || a.kc == 0) return hipSuccess;
    if ((a.dim % 4) != 0 || (a.dim_p % 64) != 0 || a.dim_p < a.dim || (a.kc_pad % 256) != 0 || a.kc_pad < a.kc || a.np == 0 || a.np > a.kc)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_screen_kernel, dim3(a.kc_pad / 64, (a.nq + 63) / 64), dim3(256), 0, s, a);
    hipLaunchKernelGGL(probe_resolve_kernel, dim3(a.nq), dim3(256), 0, s, a);
    return hipGetLastError();
}

}  // namespace pqv
