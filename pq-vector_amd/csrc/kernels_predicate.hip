// kernels_predicate.hip -- gfx950 kernels of the predicate masks (pqv.h: pqv_row_mask_from_predicates): predicate_rows_kernel
// (resident scalar columns + a postfix program -> a bitset in ROW order, the "row image"), mask_gather_kernel (row image -> the
// bitset over LIST POSITIONS that masked_stream_kernel reads; mask_layout_kernel's sibling with a bit source) and mask_pack_kernel
// (allow bytes in row order -> row image, for the byte-made masks).  All three are pure streams: no LDS, no scratch.
#include "device_common.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// predicate_rows_kernel
//
// A wave owns PRED_WORDS consecutive words of the row image, i.e. PRED_WORDS x 64 consecutive rows; lane l of word w is row
// 64 w + l, so every column read is one fully coalesced line per word.  The leaf table and the program are kernel arguments:
// wave-uniform, so the interpreter's control flow is uniform and the table is read through the scalar cache.  Each lane keeps one
// u64 bit stack per word (depth <= 32, bit 0 = top); a leaf pushes its truth, AND / OR fold the two top bits.  __ballot of the
// final top bit is the word, stored by lane 0; rows >= n_rows give zero bits.
//
// Loads in flight: a lane past the end reads row n_rows - 1 instead of nothing (the final ballot drops its bit), and whether a
// leaf has validity bytes or needs its values at all is decided once per leaf, wave-uniformly.  So no load sits under a per-lane
// branch, and the PRED_WORDS value loads and PRED_WORDS validity loads of a leaf are issued back to back before the first wait:
// 2 x PRED_WORDS requests per wave per leaf.  (Checked in the gfx950 ISA: each leaf path is a run of global_load_* and only then
// s_waitcnt vmcnt)  The program is packed into words so that a step is a scalar load, not a vector byte load.
//
// Leaf truth (pqv.h): valid && (cmp(x) != negate); IS_NULL: (!valid) != negate; MASK: bit != negate.  Integer columns compare
// in i64 (an i32 value widened), float columns in f64 (an f32 value widened, exact); the comparisons are IEEE (the unit is built
// without fast-math), so NaN fails everything but NE.
// ------------------------------------------------------------------------------------
constexpr int PRED_WORDS = 4;

template <class W>
__device__ __forceinline__ bool pred_cmp(uint32_t op, W v, W a, W b) {
    switch (op) {
    case PRED_EQ: return v == a;
    case PRED_NE: return v != a;
    case PRED_LT: return v < a;
    case PRED_LE: return v <= a;
    case PRED_GT: return v > a;
    case PRED_GE: return v >= a;
    default:      return a <= v && v <= b;       // PRED_BETWEEN
    }
}

// the truth of a comparison / IS_NULL leaf over a column of T for this lane's PRED_WORDS rows; rc[] are the lane's rows clamped
// into the column, so every load is unconditional
template <class T, class W>
__device__ __forceinline__ void pred_leaf(const PredLeaf &L, uint32_t op, bool neg, W a, W b, const uint64_t (&rc)[PRED_WORDS],
                                          bool (&t)[PRED_WORDS]) {
    const T *__restrict__ vals = static_cast<const T *>(L.values);
    const uint8_t *__restrict__ valid = L.valid;
    uint8_t ok[PRED_WORDS];
    if (op == PRED_IS_NULL) {                    // (wave-uniform: the values are not read)
        if (valid) {
#pragma unroll
            for (int u = 0; u < PRED_WORDS; ++u) ok[u] = valid[rc[u]];
#pragma unroll
            for (int u = 0; u < PRED_WORDS; ++u) t[u] = (ok[u] == 0) != neg;
        } else {
#pragma unroll
            for (int u = 0; u < PRED_WORDS; ++u) t[u] = neg;
        }
        return;
    }
    T x[PRED_WORDS];
#pragma unroll
    for (int u = 0; u < PRED_WORDS; ++u) x[u] = vals[rc[u]];
    if (valid) {                                 // (wave-uniform)
#pragma unroll
        for (int u = 0; u < PRED_WORDS; ++u) ok[u] = valid[rc[u]];
    } else {
#pragma unroll
        for (int u = 0; u < PRED_WORDS; ++u) ok[u] = 1;
    }
#pragma unroll
    for (int u = 0; u < PRED_WORDS; ++u) t[u] = ok[u] != 0 && (pred_cmp<W>(op, (W)x[u], a, b) != neg);
}

__global__ __launch_bounds__(256) void predicate_rows_kernel(const PredArgs a) {
    const int lane = threadIdx.x & 63;
    const uint64_t wave = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const uint64_t w0 = wave * PRED_WORDS;
    if (w0 >= a.n_words) return;
    const uint64_t r0 = w0 * 64 + (uint64_t)lane;

    uint64_t stk[PRED_WORDS], rc[PRED_WORDS];    // (n_words > 0 here, so n_rows > 0)
#pragma unroll
    for (int u = 0; u < PRED_WORDS; ++u) {
        stk[u] = 0;
        rc[u] = min(r0 + (uint64_t)u * 64, a.n_rows - 1);
    }

    for (uint32_t pc = 0; pc < a.program_len; ++pc) {
        const uint32_t code = (a.program[pc >> 2] >> ((pc & 3u) * 8u)) & 0xFFu;
        if (code == PRED_PROG_AND) {
#pragma unroll
            for (int u = 0; u < PRED_WORDS; ++u) stk[u] = (stk[u] >> 1) & (stk[u] | ~1ull);
        } else if (code == PRED_PROG_OR) {
#pragma unroll
            for (int u = 0; u < PRED_WORDS; ++u) stk[u] = (stk[u] >> 1) | (stk[u] & 1ull);
        } else {
            const PredLeaf &L = a.leaf[code & 31u];
            const uint32_t op = L.op & 0xFFu;
            const bool neg = (L.op & PRED_NOT) != 0;
            bool t[PRED_WORDS];
            if (op == PRED_MASK) {
                const uint64_t *__restrict__ src = static_cast<const uint64_t *>(L.values);
                uint64_t word[PRED_WORDS];
#pragma unroll
                for (int u = 0; u < PRED_WORDS; ++u) word[u] = src[rc[u] >> 6];      // (one word per 64 lanes; clamped as the rows)
#pragma unroll
                for (int u = 0; u < PRED_WORDS; ++u) t[u] = (((word[u] >> (rc[u] & 63u)) & 1ull) != 0) != neg;
            } else if (L.dtype == PRED_COL_I32) {
                pred_leaf<int32_t, int64_t>(L, op, neg, (int64_t)L.a, (int64_t)L.b, rc, t);
            } else if (L.dtype == PRED_COL_I64) {
                pred_leaf<int64_t, int64_t>(L, op, neg, (int64_t)L.a, (int64_t)L.b, rc, t);
            } else if (L.dtype == PRED_COL_F32) {
                pred_leaf<float, double>(L, op, neg, __longlong_as_double((long long)L.a), __longlong_as_double((long long)L.b), rc, t);
            } else {
                pred_leaf<double, double>(L, op, neg, __longlong_as_double((long long)L.a), __longlong_as_double((long long)L.b), rc, t);
            }
#pragma unroll
            for (int u = 0; u < PRED_WORDS; ++u) stk[u] = (stk[u] << 1) | (t[u] ? 1ull : 0ull);
        }
    }
#pragma unroll
    for (int u = 0; u < PRED_WORDS; ++u) {
        const bool on = (stk[u] & 1ull) != 0 && r0 + (uint64_t)u * 64 < a.n_rows;
        const uint64_t m = __ballot(on);
        if (lane == 0 && w0 + u < a.n_words) a.rowbits[w0 + u] = m;
    }
}

hipError_t launch_predicate_rows(const PredArgs &a, hipStream_t s) {
    if (!a.rowbits || a.program_len == 0 || a.program_len > 64) return hipErrorInvalidValue;
    const uint64_t waves = (a.n_words + PRED_WORDS - 1) / PRED_WORDS;
    const uint64_t blocks = (waves + 3) / 4;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(predicate_rows_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, a);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// mask_gather_kernel: bit p of `bits` = bit ids[p] of the row image, for list position p.  mask_layout_kernel's grid and output
// (one thread per position, one __ballot word per wave stored by lane 0, positions >= n_pos zero, every one of the n_words words
// written -- the padding word included -- and one popcount atomicAdd per wave); the ids are read coalesced, the row image is
// n_rows / 8 bytes and stays in L2.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_gather_kernel(const uint64_t *rowbits, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos,
                                                          uint64_t *bits, uint64_t n_words, unsigned long long *count) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (p < n_pos) {
        const uint64_t r = ids ? ids[p] : p;
        on = r < n_rows && ((rowbits[r >> 6] >> (r & 63u)) & 1ull) != 0;
    }
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63) == 0) {
        const uint64_t w = p >> 6;
        if (w < n_words) bits[w] = m;
        if (m) atomicAdd(count, (unsigned long long)__popcll(m));
    }
}

hipError_t launch_mask_gather(const uint64_t *rowbits, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos, uint64_t *bits,
                              uint64_t n_words, unsigned long long *count, hipStream_t s) {
    const uint64_t blocks = (n_words * 64 + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_gather_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, rowbits, n_rows, ids, n_pos, bits, n_words, count);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// mask_pack_kernel: word w of the row image = the allow bytes of rows [64 w, 64 w + 64) (nonzero = set), rows >= n_rows zero;
// all n_words words are written.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void mask_pack_kernel(const uint8_t *allowed, uint64_t n_rows, uint64_t *rowbits, uint64_t n_words) {
    const uint64_t r = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    const bool on = r < n_rows && allowed[r] != 0;
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63) == 0) {
        const uint64_t w = r >> 6;
        if (w < n_words) rowbits[w] = m;
    }
}

hipError_t launch_mask_pack(const uint8_t *allowed, uint64_t n_rows, uint64_t *rowbits, uint64_t n_words, hipStream_t s) {
    const uint64_t blocks = (n_words * 64 + 255) / 256;
    if (blocks == 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mask_pack_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, allowed, n_rows, rowbits, n_words);
    return hipGetLastError();
}

__global__ void touch_predicate_kernel() {}
hipError_t touch_predicate(hipStream_t s) {
    hipLaunchKernelGGL(touch_predicate_kernel, dim3(1), dim3(64), 0, s);
    return hipGetLastError();
}

}  // namespace pqv
