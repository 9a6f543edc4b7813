// kernels_append.hip -- list_splice_kernel: the inverted lists of an index extended by a range of new rows (pqv_index_append).
//
// The new rows were assigned and sorted by cluster already (launch_list_sort over the range: add_off[k + 1], add_rows[m] = ids local
// to the range, ascending inside a cluster).  List c of the result is list c of the old index, verbatim, followed by
// first_row + add_rows[add_off[c] ..) -- what the reference's final loop (src/ivf/index.rs:189-206) leaves for these centroids over the
// longer column, given that every new row id is above every old one.
//
// Work is cut by OUTPUT position, not by list: a block takes `per_block` consecutive positions of the result whatever the skew of
// the list lengths.  Every block first puts two tables into LDS (k <= 4096: at most 2 x 32 KB as u64): out_off[c] = old_off[c] +
// add_off[c] and old_off[c] (add_off is their difference).  A position's list is the last c with out_off[c] <= position (empty
// lists are stepped over): the block finds the lists of its first and its last position once, and a thread's search for the
// first of its four consecutive positions runs between those two -- one or two steps where lists are longer than a block's share.
// Four positions inside one source run (the old list, or the added rows) are one 16-byte load from a 4-byte aligned address and
// one aligned 16-byte store; a thread whose four positions cross a boundary walks them one by one.  64-bit offsets throughout.
#include "device_common.hpp"

namespace pqv {

__global__ __launch_bounds__(256) void list_splice_kernel(const uint64_t *__restrict__ old_off, const uint32_t *__restrict__ old_rows,
                                                          const uint64_t *__restrict__ add_off, const uint32_t *__restrict__ add_rows,
                                                          uint32_t k, uint32_t first_row, uint64_t per_block,
                                                          uint64_t *__restrict__ out_off, uint32_t *__restrict__ out_rows) {
    extern __shared__ uint64_t sp_tab[];             // [2][k + 1]: out_off, old_off
    uint64_t *const s_out = sp_tab, *const s_old = sp_tab + (k + 1);
    for (uint32_t c = threadIdx.x; c <= k; c += 256) {
        const uint64_t so = old_off[c], o = so + add_off[c];
        s_out[c] = o; s_old[c] = so;
        if (blockIdx.x == 0) out_off[c] = o;
    }
    __syncthreads();
    const uint64_t total = s_out[k];
    const uint64_t b0 = (uint64_t)blockIdx.x * per_block;      // per_block is a multiple of 4: every thread's first position is too
    uint64_t b1 = b0 + per_block;
    if (b1 > total) b1 = total;
    if (b0 >= b1) return;
    // the last c in [lo, hi) with out_off[c] <= p, given out_off[lo] <= p < out_off[hi]
    auto find = [&](uint64_t p, uint32_t lo, uint32_t hi) {
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_out[mid] <= p) lo = mid; else hi = mid;
        }
        return lo;
    };
    const uint32_t c_lo = find(b0, 0u, k), c_hi = find(b1 - 1, c_lo, k);       // (p < total = out_off[k]; block-uniform)
    for (uint64_t p = b0 + 4ull * threadIdx.x; p < b1; p += 1024) {
        uint32_t c = find(p, c_lo, c_hi + 1);
        uint64_t obeg = s_out[c], oend = s_out[c + 1];
        uint64_t sbeg = s_old[c], slen = s_old[c + 1] - sbeg, abeg = obeg - sbeg;
        const uint64_t j0 = p - obeg;
        uint32_t v[4] = {0u, 0u, 0u, 0u};
        if (p + 4 <= b1 && p + 4 <= oend && (j0 + 4 <= slen || j0 >= slen)) {
            if (j0 + 4 <= slen) {
                __builtin_memcpy(v, old_rows + sbeg + j0, 16);
            } else {
                __builtin_memcpy(v, add_rows + abeg + (j0 - slen), 16);
#pragma unroll
                for (int i = 0; i < 4; ++i) v[i] += first_row;
            }
            *reinterpret_cast<uint4 *>(out_rows + p) = make_uint4(v[0], v[1], v[2], v[3]);
            continue;
        }
        const uint32_t cnt = b1 - p < 4 ? (uint32_t)(b1 - p) : 4u;
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {           // (unrolled: v stays in registers)
            if (i < cnt) {
                const uint64_t q = p + i;
                while (q >= oend) {                  // (q < total: stops at a c < k)
                    ++c;
                    obeg = oend; oend = s_out[c + 1];
                    sbeg = s_old[c]; slen = s_old[c + 1] - sbeg; abeg = obeg - sbeg;
                }
                const uint64_t j = q - obeg;
                v[i] = j < slen ? old_rows[sbeg + j] : first_row + add_rows[abeg + (j - slen)];
            }
        }
        if (cnt == 4) {
            *reinterpret_cast<uint4 *>(out_rows + p) = make_uint4(v[0], v[1], v[2], v[3]);
        } else {
            if (cnt > 0) out_rows[p] = v[0];
            if (cnt > 1) out_rows[p + 1] = v[1];
            if (cnt > 2) out_rows[p + 2] = v[2];
        }
    }
}

// out_off[c] = old_off[c] + add_off[c] (c in [0, k]); out_rows[out_off[c] ..) = old list c, then first_row + the added rows of c.
// old_rows may be NULL when the old lists are all empty; out_rows holds old_off[k] + add_off[k] = total entries (16-byte aligned).
hipError_t launch_list_splice(const uint64_t *old_off, const uint32_t *old_rows, const uint64_t *add_off, const uint32_t *add_rows,
                              uint32_t k, uint32_t first_row, uint64_t total, uint64_t *out_off, uint32_t *out_rows, hipStream_t s) {
    if (k == 0 || k > 4096 || !old_off || !add_off || !out_off || (total && (!add_rows || !out_rows)) ||
        (reinterpret_cast<uintptr_t>(out_rows) & 15u) != 0)
        return hipErrorInvalidValue;
    const size_t lds = 2 * (size_t)(k + 1) * sizeof(uint64_t);
    if (lds > 49152) {          // (more than 3071 clusters: asked for per call -- the attribute belongs to the current device's copy of the kernel)
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(list_splice_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    }
    // a block fills the two offset tables (k + 1 entries each) before it copies: at least 4096 positions, and 4 per table
    // entry, per block; at most 2048 blocks
    uint64_t per_block = 4096 > 4ull * (k + 1) ? 4096 : 4ull * (k + 1);
    if ((total + per_block - 1) / per_block > 2048) per_block = (total + 2047) / 2048;
    per_block = (per_block + 3) / 4 * 4;
    const uint64_t blocks = total ? (total + per_block - 1) / per_block : 1;
    hipLaunchKernelGGL(list_splice_kernel, dim3((uint32_t)blocks), dim3(256), lds, s, old_off, old_rows, add_off, add_rows, k, first_row,
                       per_block, out_off, out_rows);
    return hipGetLastError();
}

}  // namespace pqv
