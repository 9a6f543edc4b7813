// kernels_expand.hip -- gfx950 kernels of the expanding filtered top-k (pqv.h: pqv_topk_expand): filter_count_kernel (how many
// positions of each probed list pass the call's filter -- no embedding is read) and expand_select_kernel (per query: the prefix
// sums of those counts in probe order, the first rank at which k rows have passed, the candidate total of the lists up to it).
// masked_stream_kernel (kernels_mask.hip) then walks each query's lists below its own rank limit.
// Also the depth stage of the plain call under per-query depths (pqv.h: pqv_topk_depth): probe_depth_kernel, depth_seed_clear_kernel.
#include "stream_walk.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// filter_count_kernel<WIN>: grid (probe rank j < P, query), one 256-thread block per probed list; cnt[q * P + j] = the set bits of
// the list's windows, ONE plain store per block, no atomics.
//
// A window's 64 bits are masked_stream_kernel's for the same WIN, from the same KeyTest (stream_walk.hpp): positions
// lbeg + w0 .. + 63 of the list, w0 a multiple of 64 -- the stream's waves start their ranges at multiples of 64 inside the
// list and clip at min(range end, list end), so the union of their windows is exactly these, clipped at the list's end.
// WIN 0: the mask's image through image_window.  WIN 1 .. 6: lane l loads key_pos[lbeg + w0 + l], compares in i64 (equality /
// inclusive range / a halving search in the query's set, copied into LDS first) and the __ballot is the window, ANDed with the
// windows of valid_pos and of the shared mask where the call has them.  No candidate cap: an expanding call takes none.
//
// WIN 0 needs no ballot, so every LANE takes a window of its own (a block covers 16 K positions per turn); the keyed forms take
// one window per wave and turn, the four waves striding over the list.  Per-thread sums, one wave reduction, four words of LDS.
// An empty IN slice counts 0 without reading a key.
// ------------------------------------------------------------------------------------
template <int WIN>
__global__ __launch_bounds__(256) void filter_count_kernel(const ExpandCountArgs a) {
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.y, j = blockIdx.x;
    const uint32_t c = a.probe[(uint64_t)q * a.P + j];
    const uint64_t lbeg = a.list_off[c], len = a.list_off[c + 1] - lbeg;

    __shared__ uint32_t s_sum[4];
    uint32_t sum = 0;           // WIN 0: this lane's windows; else wave-uniform
    if constexpr (WIN == 0) {
        for (uint64_t w0 = (uint64_t)threadIdx.x * 64; w0 < len; w0 += 256 * 64) {
            uint64_t win = image_window(a.bits, lbeg + w0);
            if (len - w0 < 64) win &= (1ull << (len - w0)) - 1ull;
            sum += (uint32_t)__popcll(win);
        }
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) sum += (uint32_t)__shfl_xor((int)sum, d, 64);
    } else {
        KeyTest<(WIN - 1) / 2> kt;          // WIN 1 / 2: EQ, 3 / 4: RANGE, 5 / 6: IN
        if constexpr (WIN <= 4) kt.lo = static_cast<const int64_t *>(a.a)[q];
        if constexpr (WIN == 3 || WIN == 4) kt.hi = static_cast<const int64_t *>(a.b)[q];
        uint64_t end = len;
        if constexpr (WIN >= 5) {
            __shared__ int64_t set_lds[KEY_SET_MAX];
            kt.setup_in(a.a, a.b, q, set_lds);
            if (kt.empty()) end = 0;       // (nothing matches: no window is read)
        }
        for (uint64_t w0 = (uint64_t)wave * 64; w0 < end; w0 += 256) {
            const uint64_t p = lbeg + w0;
            uint64_t win = kt.window(a.key_pos, (WIN & 1) != 0, a.valid_pos, p, lane);      // (positions >= len are clipped below)
            if (a.bits) win &= image_window(a.bits, p);
            if (len - w0 < 64) win &= (1ull << (len - w0)) - 1ull;
            sum += (uint32_t)__popcll(win);
        }
    }
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) a.cnt[(uint64_t)q * a.P + j] = s_sum[0] + s_sum[1] + s_sum[2] + s_sum[3];
}

hipError_t launch_filter_count(const ExpandCountArgs &a, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cnt) return hipErrorInvalidValue;
    if (a.nq == 0 || a.P == 0) return hipSuccess;
    if (a.nq > 65535u) return hipErrorInvalidValue;
    const dim3 grid(a.P, a.nq), block(256);
    if (a.win == 0) {
        if (!a.bits) return hipErrorInvalidValue;
        hipLaunchKernelGGL(filter_count_kernel<0>, grid, block, 0, s, a);
        return hipGetLastError();
    }
    if (!a.key_pos || !a.a || a.win > 6 || (a.win >= 3 && !a.b)) return hipErrorInvalidValue;
    switch (a.win) {
        case 1: hipLaunchKernelGGL(filter_count_kernel<1>, grid, block, 0, s, a); break;
        case 2: hipLaunchKernelGGL(filter_count_kernel<2>, grid, block, 0, s, a); break;
        case 3: hipLaunchKernelGGL(filter_count_kernel<3>, grid, block, 0, s, a); break;
        case 4: hipLaunchKernelGGL(filter_count_kernel<4>, grid, block, 0, s, a); break;
        case 5: hipLaunchKernelGGL(filter_count_kernel<5>, grid, block, 0, s, a); break;
        default: hipLaunchKernelGGL(filter_count_kernel<6>, grid, block, 0, s, a); break;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// expand_select_kernel: one wave per query.  The inclusive prefix sums of cnt[q][0 .. P) in chunks of 64 ranks -- a wave scan in
// 64 bits (a list position is below 2^32, the sum of 1024 lists need not be), the carry wave-uniform -- and the first rank j in
// [p0 - 1, P) whose prefix is >= k: used = j + 1, or P where there is none.  Lane 0 writes nprobe_used[q] = used and OVERWRITES
// n_cand[q] (the probe merge's total over all P lists) with the total of the first `used`: cand_base of the last one plus its length.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void expand_select_kernel(const ExpandSelectArgs a) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint32_t *cnt = a.cnt + (uint64_t)q * a.P;
    uint64_t carry = 0;
    uint32_t used = a.P;
    for (uint32_t c0 = 0; c0 < a.P; c0 += 64) {
        const uint32_t j = c0 + (uint32_t)lane;
        uint64_t v = j < a.P ? (uint64_t)cnt[j] : 0ull;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
            const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
            if (lane >= d) v += ((uint64_t)hi << 32) | lo;
        }
        v += carry;
        const unsigned long long hit = __ballot(j < a.P && j + 1 >= a.p0 && v >= (uint64_t)a.k);
        if (hit) { used = c0 + (uint32_t)__builtin_ctzll(hit) + 1u; break; }
        carry = readlane_u64(v, 63);
    }
    if (lane == 0) {
        a.nprobe_used[q] = used;
        const uint64_t at = (uint64_t)q * a.P + (used - 1);
        const uint32_t c = a.probe[at];
        a.n_cand[q] = a.cand_base[at] + (a.list_off[c + 1] - a.list_off[c]);
    }
}

hipError_t launch_expand_select(const ExpandSelectArgs &a, hipStream_t s) {
    if (!a.cnt || !a.probe || !a.cand_base || !a.list_off || !a.nprobe_used || !a.n_cand) return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    if (a.P == 0 || a.p0 == 0 || a.p0 > a.P) return hipErrorInvalidValue;
    hipLaunchKernelGGL(expand_select_kernel, dim3(a.nq), dim3(64), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// probe_depth_kernel (pqv.h: pqv_topk_depth): one wave per query.  The raw depth is the caller's, or the ranks whose probe
// distance is at most t = ratio * d2_0 -- ONE f32 multiplication (the unit is built without contraction) and an ordered <=, so a
// NaN threshold (inf * 0) or a NaN distance counts nothing; the distances ascend, so the counted ranks are a prefix.  Clamped into
// [p0, P].  Lane 0 writes nprobe_used[q], OVERWRITES n_cand[q] as expand_select_kernel does and counts it; the wave writes every
// pair's candidate end (ProbeDepthArgs::pair_end) and adds the pairs below the depth to the pair sort's cluster histogram, which the
// probe merge of such a call leaves empty.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void probe_depth_kernel(const ProbeDepthArgs a) {
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint64_t row = (uint64_t)q * a.P;
    uint32_t r = 0;
    if (a.depths) {
        r = a.depths[q];
    } else {
        const float t = a.ratio * __uint_as_float(a.d2[row]);
        for (uint32_t c0 = 0; c0 < a.P; c0 += 64) {
            const uint32_t j = c0 + (uint32_t)lane;
            const bool in = j < a.P && __uint_as_float(a.d2[row + (j < a.P ? j : 0u)]) <= t;
            r += (uint32_t)__popcll(__ballot(in));
        }
    }
    uint32_t used = r < a.p0 ? a.p0 : r;
    if (used > a.P) used = a.P;
    for (uint32_t j = (uint32_t)lane; j < a.P; j += 64) {
        a.pair_end[row + j] = j < used ? ~0ull : 0ull;
        if (a.hist && j < used) atomicAdd(&a.hist[(uint64_t)(q % HIST_REPLICAS) * a.hist_stride + a.probe[row + j]], 1u);
    }
    if (lane == 0) {
        a.nprobe_used[q] = used;
        const uint64_t at = row + (used - 1);
        const uint32_t c = a.probe[at];
        const uint64_t total = a.cand_base[at] + (a.list_off[c + 1] - a.list_off[c]);
        a.n_cand[q] = total;
        if (unsigned long long *st = stats_slot(a.stats, q)) {
            atomicAdd(&st[2], (unsigned long long)total);
            atomicAdd(&st[3], (unsigned long long)total);
        }
    }
}

hipError_t launch_probe_depth(const ProbeDepthArgs &a, hipStream_t s) {
    if (!(a.depths || a.d2) || !a.probe || !a.cand_base || !a.list_off || !a.nprobe_used || !a.n_cand || !a.pair_end) return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    if (a.P == 0 || a.p0 == 0 || a.p0 > a.P) return hipErrorInvalidValue;
    hipLaunchKernelGGL(probe_depth_kernel, dim3(a.nq), dim3(64), 0, s, a);
    return hipGetLastError();
}

// one block per query: the seed bounds of its ranks [rank_limit[q], P) are one contiguous run of (P - limit) * per_rank floats
__global__ __launch_bounds__(256) void depth_seed_clear_kernel(float *seed_ub, const uint32_t *rank_limit, uint32_t P, uint32_t per_rank) {
    const uint32_t q = blockIdx.x;
    const uint32_t lim = rank_limit[q] < P ? rank_limit[q] : P;
    float *dst = seed_ub + ((uint64_t)q * P + lim) * per_rank;
    const uint64_t n = (uint64_t)(P - lim) * per_rank;
    for (uint64_t i = threadIdx.x; i < n; i += 256) dst[i] = INFINITY;
}

hipError_t launch_depth_seed_clear(float *seed_ub, const uint32_t *rank_limit, uint32_t nq, uint32_t P, uint32_t per_rank, hipStream_t s) {
    if (!seed_ub || !rank_limit) return hipErrorInvalidValue;
    if (nq == 0 || P == 0 || per_rank == 0) return hipSuccess;
    hipLaunchKernelGGL(depth_seed_clear_kernel, dim3(nq), dim3(256), 0, s, seed_ub, rank_limit, P, per_rank);
    return hipGetLastError();
}

}  // namespace pqv
