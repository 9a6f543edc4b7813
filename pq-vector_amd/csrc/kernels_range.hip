// kernels_range.hip -- gfx950 kernels behind the range search (pqv_range_search): the per-query hit segments that
// stream_kernel's STREAM_RANGE mode appends to are put into (d2, candidate position) order -- a key unique per query, so
// the answer does not depend on the order in which the waves appended -- and written out as rows and distances.
//   range_sort_small_kernel   0 < n <= RANGE_SMALL: one block sorts the segment in LDS (bitonic) and writes it out
//   range_tile_sort_kernel    longer segments: every RANGE_SMALL-key tile sorted in place
//   range_merge_kernel        ... then sorted runs of width w merged pairwise into runs of 2w (merge path, 8 outputs a
//                             thread), ping-pong between the segment buffer and a compact second buffer
//   range_write_kernel        ... and the first min(n, max_results) entries written out
// A segment begins at range_seg_base(seg_off, seg_stride, q): q * seg_stride, or -- the partition range search's packed segments --
// seg_off[q].
#include "device_common.hpp"

namespace pqv {

namespace {

constexpr uint32_t RS_THREADS = 1024;     // (a 4096-key bitonic sort: 2 compare-exchanges per thread and stage)
constexpr uint32_t RS_ITEMS = 8;        // outputs per thread of a merge pass

// ascending bitonic sort of sk / sv [0, n2) in LDS (n2 a power of two >= 2), by the whole block
__device__ __forceinline__ void block_bitonic_sort(uint64_t *sk, uint32_t *sv, uint32_t n2) {
    for (uint32_t k2 = 2; k2 <= n2; k2 <<= 1) {
        for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
            for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
                const uint32_t ixj = i ^ j;
                if (ixj > i) {
                    const uint64_t a = sk[i], b = sk[ixj];
                    const bool up = (i & k2) == 0;
                    if ((a > b) == up) {
                        sk[i] = b; sk[ixj] = a;
                        const uint32_t t = sv[i]; sv[i] = sv[ixj]; sv[ixj] = t;
                    }
                }
            }
            __syncthreads();
        }
    }
}

__device__ __forceinline__ uint32_t pow2_at_least(uint32_t n) {
    uint32_t p = 2;
    while (p < n) p <<= 1;
    return p;
}

__device__ __forceinline__ void write_hit(const RangeSortArgs &a, uint64_t o, uint64_t key, uint32_t val) {
    const float d2 = __uint_as_float((uint32_t)(key >> 32));
    a.out_rows[o] = a.ids ? a.ids[val] : val;
    a.out_dist[o] = a.sqrt_out == 1 ? sqrt_f32_ieee(d2) : a.sqrt_out == 2 ? 0.5f * d2 : d2;     // search.rs:133; 2: PQV_COSINE
}

__device__ __forceinline__ uint64_t kept_of(const RangeSortArgs &a, uint32_t n) {
    return (a.max_results && a.max_results < n) ? a.max_results : n;
}

}  // namespace

__global__ __launch_bounds__(RS_THREADS) void range_sort_small_kernel(const RangeSortArgs a) {
    __shared__ uint64_t sk[RANGE_SMALL];
    __shared__ uint32_t sv[RANGE_SMALL];
    const uint32_t q = blockIdx.x;
    const uint32_t n = a.hit_cnt[q];
    if (n == 0 || n > RANGE_SMALL) return;
    const uint32_t n2 = pow2_at_least(n);
    const uint64_t seg = range_seg_base(a.seg_off, a.seg_stride, q);
    const uint64_t *gk = a.keys + seg;
    const uint32_t *gv = a.vals + seg;
    for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
        sk[i] = i < n ? gk[i] : KEY_EMPTY;
        sv[i] = i < n ? gv[i] : 0xFFFFFFFFu;
    }
    __syncthreads();
    block_bitonic_sort(sk, sv, n2);
    const uint64_t kept = kept_of(a, n), o = a.out_off[q];
    for (uint32_t i = threadIdx.x; i < kept; i += blockDim.x) write_hit(a, o + i, sk[i], sv[i]);
}

// grid (tiles of the longest segment, n_segs): tile blockIdx.x of segment blockIdx.y, sorted in place in the segment buffer
__global__ __launch_bounds__(RS_THREADS) void range_tile_sort_kernel(const RangeSortArgs a) {
    __shared__ uint64_t sk[RANGE_SMALL];
    __shared__ uint32_t sv[RANGE_SMALL];
    const RangeSeg sg = a.segs[blockIdx.y];
    const uint64_t t0 = (uint64_t)blockIdx.x * RANGE_SMALL;
    if (t0 >= sg.n) return;
    const uint32_t m = (uint32_t)((sg.n - t0 < RANGE_SMALL) ? sg.n - t0 : RANGE_SMALL);
    const uint64_t seg = range_seg_base(a.seg_off, a.seg_stride, sg.q);
    uint64_t *gk = a.keys + seg + t0;
    uint32_t *gv = a.vals + seg + t0;
    const uint32_t n2 = pow2_at_least(m);
    for (uint32_t i = threadIdx.x; i < n2; i += blockDim.x) {
        sk[i] = i < m ? gk[i] : KEY_EMPTY;
        sv[i] = i < m ? gv[i] : 0xFFFFFFFFu;
    }
    __syncthreads();
    block_bitonic_sort(sk, sv, n2);
    for (uint32_t i = threadIdx.x; i < m; i += blockDim.x) { gk[i] = sk[i]; gv[i] = sv[i]; }
}

// grid (ceil(longest / (RS_THREADS * RS_ITEMS)), n_segs): runs [2iw, 2iw + w) and [2iw + w, 2iw + 2w) of the source merged
// into [2iw, 2iw + 2w) of the destination; to_alt: segment buffer -> second buffer, else back
__global__ __launch_bounds__(RS_THREADS) void range_merge_kernel(const RangeSortArgs a, uint32_t w, int to_alt) {
    const RangeSeg sg = a.segs[blockIdx.y];
    const uint64_t n = sg.n;
    const uint64_t o0 = ((uint64_t)blockIdx.x * RS_THREADS + threadIdx.x) * RS_ITEMS;
    if (o0 >= n) return;
    const uint64_t seg = range_seg_base(a.seg_off, a.seg_stride, sg.q);
    uint64_t *mk = a.keys + seg;
    uint32_t *mv = a.vals + seg;
    uint64_t *xk = a.alt_keys + sg.alt_off;
    uint32_t *xv = a.alt_vals + sg.alt_off;
    const uint64_t *sk = to_alt ? mk : xk;
    const uint32_t *sv = to_alt ? mv : xv;
    uint64_t *dk = to_alt ? xk : mk;
    uint32_t *dv = to_alt ? xv : mv;
    const uint64_t ps = o0 / (2ull * w) * (2ull * w);
    const uint64_t a_end = ps + w < n ? ps + w : n;
    const uint64_t b_end = ps + 2ull * w < n ? ps + 2ull * w : n;
    const uint64_t la = a_end - ps, lb = b_end - a_end;
    const uint64_t *ka = sk + ps, *kb = sk + a_end;
    // merge path: i entries of run A and d - i of run B precede output d (keys are distinct)
    const uint64_t d = o0 - ps;
    uint64_t lo = d > lb ? d - lb : 0, hi = d < la ? d : la;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (ka[mid] < kb[d - 1 - mid]) lo = mid + 1; else hi = mid;
    }
    uint64_t i = lo, j = d - lo;
    const uint64_t end = o0 + RS_ITEMS < b_end ? o0 + RS_ITEMS : b_end;
    for (uint64_t o = o0; o < end; ++o) {
        const bool take_a = j >= lb || (i < la && ka[i] < kb[j]);
        if (take_a) { dk[o] = ka[i]; dv[o] = sv[ps + i]; ++i; }
        else { dk[o] = kb[j]; dv[o] = sv[a_end + j]; ++j; }
    }
}

// grid (ceil(longest kept / RS_THREADS), n_segs): the sorted segment (in the second buffer if from_alt) written out
__global__ __launch_bounds__(RS_THREADS) void range_write_kernel(const RangeSortArgs a, int from_alt) {
    const RangeSeg sg = a.segs[blockIdx.y];
    const uint64_t i = (uint64_t)blockIdx.x * RS_THREADS + threadIdx.x;
    if (i >= kept_of(a, sg.n)) return;
    const uint64_t src = from_alt ? sg.alt_off + i : range_seg_base(a.seg_off, a.seg_stride, sg.q) + i;
    write_hit(a, a.out_off[sg.q] + i, from_alt ? a.alt_keys[src] : a.keys[src], from_alt ? a.alt_vals[src] : a.vals[src]);
}

hipError_t launch_range_sort_small(const RangeSortArgs &a, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    hipLaunchKernelGGL(range_sort_small_kernel, dim3(a.nq), dim3(RS_THREADS), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_range_sort_large(const RangeSortArgs &a, uint32_t max_n, uint32_t *launches, hipStream_t s) {
    *launches = 0;
    if (a.n_segs == 0 || max_n == 0) return hipSuccess;
    if (a.n_segs > 65535) return hipErrorInvalidValue;          // (gridDim.y; the caller's sub-batches are smaller)
    hipLaunchKernelGGL(range_tile_sort_kernel, dim3((max_n + RANGE_SMALL - 1) / RANGE_SMALL, a.n_segs), dim3(RS_THREADS), 0, s, a);
    if (hipError_t e = hipGetLastError()) return e;
    ++*launches;
    const uint32_t per_block = RS_THREADS * RS_ITEMS;
    int in_alt = 0;
    for (uint64_t w = RANGE_SMALL; w < max_n; w *= 2) {
        hipLaunchKernelGGL(range_merge_kernel, dim3((max_n + per_block - 1) / per_block, a.n_segs), dim3(RS_THREADS), 0, s, a,
                           (uint32_t)w, in_alt ? 0 : 1);
        if (hipError_t e = hipGetLastError()) return e;
        ++*launches;
        in_alt ^= 1;
    }
    uint64_t max_kept = a.max_results && a.max_results < max_n ? a.max_results : max_n;
    hipLaunchKernelGGL(range_write_kernel, dim3((uint32_t)((max_kept + RS_THREADS - 1) / RS_THREADS), a.n_segs), dim3(RS_THREADS), 0, s,
                       a, in_alt);
    ++*launches;
    return hipGetLastError();
}

__global__ void touch_range_kernel() {}
hipError_t touch_range(hipStream_t s) {
    hipLaunchKernelGGL(touch_range_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace pqv
