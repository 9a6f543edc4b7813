// kernels_remove.hip -- the device side of pqv_index_remove / pqv_index_compact: ranking over a bitset, and what is built on it.
//
// A bitset (one bit per list position, or one bit per row id) says which entries stay.  bit_rank turns it into the exclusive
// prefix of its per-word popcounts, one u64 per word plus the total behind the last word, so that
//     rank_at(p) = rank[p >> 6] + popcount(word(p >> 6) & below(p & 63))
// is the number of set bits below p: the output slot of a kept list position (remove), the new id of a kept row (compact).
// The "effective" word of a bitset is word_of(): the stored word, inverted where the stored bits mark what LEAVES (remove reuses
// launch_mask_layout unchanged: its bit p = "the flag byte of the row at position p is non-zero" = removed), and cut at n_bits.
//
//   bit_rank_sums_kernel / bit_rank_scan_kernel / bit_rank_final_kernel   block sums, their scan (one block), the final pass
//   list_compact_kernel    out[rank_at(p)] = ids ? ids[p] : p for every kept p -- the lists without the removed rows; with
//                          ids == NULL over row space, old_row[new id] = old id
//   offsets_rank_kernel    new_off[c] = rank_at(old_off[c]), c in [0, k]: one thread per entry, no table in LDS, no cluster limit
//   member_bytes_kernel    member[id] = 1 for every id in the lists (byte stores; duplicates collapse), ids >= n_rows flagged
//   lists_remap_kernel     out[p] = rank_at(ids[p]) over row space
//   rows_gather_kernel     dst row j = src row old_row[j]: 16-byte nt loads and stores (dim % 4 == 0), else dword ones
//
// Work is cut by INPUT position everywhere (a thread owns four consecutive positions, one 16-byte load of ids), so the skew of
// the list lengths does not matter.  Plain vector stores only; 64-bit offsets throughout; no LDS beyond the block scans' 4 words.
#include "device_common.hpp"

namespace pqv {

namespace {

constexpr uint32_t RANK_WORDS_PER_THREAD = 4;
constexpr uint32_t RANK_WORDS_PER_BLOCK = 256 * RANK_WORDS_PER_THREAD;       // 65536 bits per block

// the effective word w of a bitset of n_bits bits (w < ceil(n_bits / 64)): inverted if the stored bits mark removals, bits at
// or beyond n_bits zero
__device__ __forceinline__ uint64_t word_of(const uint64_t *__restrict__ bits, uint64_t w, uint64_t n_bits, uint32_t invert) {
    uint64_t v = bits[w];
    if (invert) v = ~v;
    const uint64_t left = n_bits - (w << 6);          // > 0
    if (left < 64) v &= (1ull << left) - 1ull;
    return v;
}

// set bits below position p (p <= n_bits); rank[n_words] is the total
__device__ __forceinline__ uint64_t rank_at(const uint64_t *__restrict__ bits, const uint64_t *__restrict__ rank, uint64_t p,
                                            uint64_t n_bits, uint32_t invert) {
    if (p >= n_bits) return rank[(n_bits + 63) >> 6];
    const uint64_t w = p >> 6;
    const uint64_t below = (1ull << (p & 63)) - 1ull;
    return rank[w] + (uint64_t)__popcll(word_of(bits, w, n_bits, invert) & below);
}

// exclusive prefix of v over the 256 threads of a block, and the block's total (wave64 shuffles + one LDS word per wave)
__device__ __forceinline__ uint32_t block_excl_scan(uint32_t v, uint32_t *total) {
    __shared__ uint32_t wave_sum[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t up = __shfl_up(inc, d, 64);
        if (lane >= d) inc += up;
    }
    if (lane == 63) wave_sum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const uint32_t s = wave_sum[i];
        if (i < wave) base += s;
        tot += s;
    }
    __syncthreads();                                  // (wave_sum may be written again by the caller's next scan)
    *total = tot;
    return base + inc - v;
}

__device__ __forceinline__ uint32_t thread_words(const uint64_t *__restrict__ bits, uint64_t n_words, uint64_t n_bits, uint32_t invert,
                                                 uint64_t w0, uint32_t cnt[RANK_WORDS_PER_THREAD]) {
    uint32_t sum = 0;
#pragma unroll
    for (uint32_t i = 0; i < RANK_WORDS_PER_THREAD; ++i) {
        const uint64_t w = w0 + i;
        cnt[i] = w < n_words ? (uint32_t)__popcll(word_of(bits, w, n_bits, invert)) : 0u;
        sum += cnt[i];
    }
    return sum;
}

}  // namespace

// block_sum[b] = set bits of the block's RANK_WORDS_PER_BLOCK words
__global__ __launch_bounds__(256) void bit_rank_sums_kernel(const uint64_t *__restrict__ bits, uint64_t n_words, uint64_t n_bits,
                                                            uint32_t invert, uint64_t *__restrict__ block_sum) {
    const uint64_t w0 = (uint64_t)blockIdx.x * RANK_WORDS_PER_BLOCK + (uint64_t)threadIdx.x * RANK_WORDS_PER_THREAD;
    uint32_t cnt[RANK_WORDS_PER_THREAD];
    const uint32_t mine = thread_words(bits, n_words, n_bits, invert, w0, cnt);
    uint32_t total = 0;
    (void)block_excl_scan(mine, &total);
    if (threadIdx.x == 0) block_sum[blockIdx.x] = total;
}

// in place: block_sum[b] -> the sum of the blocks before b; *total = the sum of all (ONE block of 256 threads walks the array)
__global__ __launch_bounds__(256) void bit_rank_scan_kernel(uint64_t *__restrict__ block_sum, uint64_t n_blocks, uint64_t *__restrict__ total) {
    uint64_t carry = 0;
    for (uint64_t b0 = 0; b0 < n_blocks; b0 += 256) {
        const uint64_t b = b0 + threadIdx.x;
        const uint32_t v = b < n_blocks ? (uint32_t)block_sum[b] : 0u;          // (a block's sum is at most 65536)
        uint32_t tot = 0;
        const uint32_t ex = block_excl_scan(v, &tot);
        if (b < n_blocks) block_sum[b] = carry + ex;
        carry += tot;
    }
    if (threadIdx.x == 0) *total = carry;
}

// rank[w] = set bits of the words before w (w < n_words); rank[n_words] was written by the scan
__global__ __launch_bounds__(256) void bit_rank_final_kernel(const uint64_t *__restrict__ bits, uint64_t n_words, uint64_t n_bits,
                                                             uint32_t invert, const uint64_t *__restrict__ block_base,
                                                             uint64_t *__restrict__ rank) {
    const uint64_t w0 = (uint64_t)blockIdx.x * RANK_WORDS_PER_BLOCK + (uint64_t)threadIdx.x * RANK_WORDS_PER_THREAD;
    uint32_t cnt[RANK_WORDS_PER_THREAD];
    const uint32_t mine = thread_words(bits, n_words, n_bits, invert, w0, cnt);
    uint32_t total = 0;
    uint64_t at = block_base[blockIdx.x] + block_excl_scan(mine, &total);
#pragma unroll
    for (uint32_t i = 0; i < RANK_WORDS_PER_THREAD; ++i) {
        if (w0 + i < n_words) rank[w0 + i] = at;
        at += cnt[i];
    }
}

// A thread owns positions [p, p + 4), p a multiple of 4: all four lie in one word.  Kept entries go to consecutive slots from
// rank_at(p); a wave's 256 positions are four words, so its kept ids land in one contiguous run of the output.
__global__ __launch_bounds__(256) void list_compact_kernel(const uint32_t *__restrict__ ids, uint64_t n_pos, const uint64_t *__restrict__ bits,
                                                           uint32_t invert, const uint64_t *__restrict__ rank, uint32_t *__restrict__ out) {
    const uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= n_pos) return;
    const uint64_t w = p >> 6;
    const uint32_t sh = (uint32_t)(p & 63);
    const uint64_t word = word_of(bits, w, n_pos, invert);
    const uint32_t keep = (uint32_t)(word >> sh) & 15u;          // (positions >= n_pos are zero bits)
    if (!keep) return;
    uint32_t v[4] = {(uint32_t)p, (uint32_t)p + 1u, (uint32_t)p + 2u, (uint32_t)p + 3u};
    if (ids) {
        if (p + 4 <= n_pos) {
            __builtin_memcpy(v, ids + p, 16);
        } else {
#pragma unroll
            for (uint32_t i = 0; i < 4; ++i) v[i] = p + i < n_pos ? ids[p + i] : 0u;
        }
    }
    uint64_t slot = rank[w] + (uint64_t)__popcll(word & ((1ull << sh) - 1ull));
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i)
        if (keep & (1u << i)) out[slot++] = v[i];
}

__global__ __launch_bounds__(256) void offsets_rank_kernel(const uint64_t *__restrict__ old_off, uint32_t n_entries, const uint64_t *__restrict__ bits,
                                                           uint64_t n_pos, uint32_t invert, const uint64_t *__restrict__ rank,
                                                           uint64_t *__restrict__ new_off) {
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    if (c >= n_entries) return;
    new_off[c] = rank_at(bits, rank, old_off[c], n_pos, invert);
}

__global__ __launch_bounds__(256) void member_bytes_kernel(const uint32_t *__restrict__ ids, uint64_t n_pos, uint64_t n_rows,
                                                           uint8_t *__restrict__ member, uint32_t *__restrict__ bad) {
    const uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= n_pos) return;
    uint32_t v[4];
    uint32_t cnt = 4;
    if (p + 4 <= n_pos) {
        __builtin_memcpy(v, ids + p, 16);
    } else {
        cnt = (uint32_t)(n_pos - p);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) v[i] = i < cnt ? ids[p + i] : 0u;
    }
    bool out_of_range = false;
#pragma unroll
    for (uint32_t i = 0; i < 4; ++i) {
        if (i < cnt) {
            if (v[i] < n_rows) member[v[i]] = 1;
            else out_of_range = true;
        }
    }
    if (out_of_range) atomicOr(bad, 1u);
}

// out[p] = the rank of row ids[p] among the member rows (every id is a member and below n_rows: checked by the caller)
__global__ __launch_bounds__(256) void lists_remap_kernel(const uint32_t *__restrict__ ids, uint64_t n_pos, const uint64_t *__restrict__ rowbits,
                                                          uint64_t n_rows, const uint64_t *__restrict__ rank, uint32_t *__restrict__ out) {
    const uint64_t p = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (p >= n_pos) return;
    if (p + 4 <= n_pos) {
        uint32_t v[4];
        __builtin_memcpy(v, ids + p, 16);
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) v[i] = v[i] < n_rows ? (uint32_t)rank_at(rowbits, rank, v[i], n_rows, 0u) : 0u;
        *reinterpret_cast<uint4 *>(out + p) = make_uint4(v[0], v[1], v[2], v[3]);
        return;
    }
    for (uint64_t q = p; q < n_pos; ++q) {
        const uint32_t r = ids[q];
        out[q] = r < n_rows ? (uint32_t)rank_at(rowbits, rank, r, n_rows, 0u) : 0u;
    }
}

// The rows as one flat run of granules (T = a 16-byte vector where dim % 4 == 0 and both bases are 16-byte aligned, else one f32),
// g granules per row: a block takes 1024 consecutive granules of the OUTPUT, a thread four of them 256 apart -- several rows per
// block where rows are short, a row cut over the block (and over blocks) where they are long; four loads are in flight before
// the first store.  The block's first row and column come from one 64-bit division, a thread's from 32-bit ones.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <class T>
__global__ __launch_bounds__(256) void rows_gather_kernel(const T *__restrict__ src, const uint32_t *__restrict__ old_row, uint64_t m, uint32_t g,
                                                          T *__restrict__ dst) {
    const uint64_t total = m * g;
    const uint64_t i0 = (uint64_t)blockIdx.x * 1024;
    const uint64_t row0 = i0 / g;
    const uint32_t col0 = (uint32_t)(i0 - row0 * g);
    T v[4];
    bool on[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) {
        const uint32_t local = j * 256 + threadIdx.x;
        on[j] = i0 + local < total;
        if (on[j]) {
            const uint32_t lc = local + col0;             // < 1024 + g <= 2^31
            const uint32_t dr = lc / g, col = lc - dr * g;
            const uint64_t r = old_row[row0 + dr];
            v[j] = __builtin_nontemporal_load(src + r * g + col);
        }
    }
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j)
        if (on[j]) __builtin_nontemporal_store(v[j], dst + i0 + j * 256 + threadIdx.x);
}

// ------------------------------------------------------------------------------------ launchers
static inline uint64_t quads_blocks(uint64_t n_pos) { return (n_pos + 1023) / 1024; }

uint64_t bit_rank_blocks(uint64_t n_bits) {
    const uint64_t n_words = (n_bits + 63) / 64;
    return (n_words + RANK_WORDS_PER_BLOCK - 1) / RANK_WORDS_PER_BLOCK;
}

hipError_t launch_bit_rank(const uint64_t *bits, uint64_t n_bits, bool invert, uint64_t *rank, uint64_t *block_tmp, hipStream_t s) {
    if (!rank || !block_tmp || (n_bits && !bits)) return hipErrorInvalidValue;
    const uint64_t n_words = (n_bits + 63) / 64, blocks = bit_rank_blocks(n_bits);
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (blocks)
        hipLaunchKernelGGL(bit_rank_sums_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, bits, n_words, n_bits, invert ? 1u : 0u, block_tmp);
    hipLaunchKernelGGL(bit_rank_scan_kernel, dim3(1), dim3(256), 0, s, block_tmp, blocks, rank + n_words);
    if (blocks)
        hipLaunchKernelGGL(bit_rank_final_kernel, dim3((uint32_t)blocks), dim3(256), 0, s, bits, n_words, n_bits, invert ? 1u : 0u, block_tmp, rank);
    return hipGetLastError();
}

hipError_t launch_list_compact(const uint32_t *ids, uint64_t n_pos, const uint64_t *bits, bool invert, const uint64_t *rank, uint32_t *out,
                               hipStream_t s) {
    if (n_pos == 0) return hipSuccess;
    if (!bits || !rank || !out || n_pos > (1ull << 32) || (reinterpret_cast<uintptr_t>(ids) & 3u) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(list_compact_kernel, dim3((uint32_t)quads_blocks(n_pos)), dim3(256), 0, s, ids, n_pos, bits, invert ? 1u : 0u, rank, out);
    return hipGetLastError();
}

hipError_t launch_offsets_rank(const uint64_t *old_off, uint32_t n_entries, const uint64_t *bits, uint64_t n_pos, bool invert,
                               const uint64_t *rank, uint64_t *new_off, hipStream_t s) {
    if (n_entries == 0) return hipSuccess;
    if (!old_off || !rank || !new_off || (n_pos && !bits)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(offsets_rank_kernel, dim3((n_entries + 255) / 256), dim3(256), 0, s, old_off, n_entries, bits, n_pos, invert ? 1u : 0u,
                       rank, new_off);
    return hipGetLastError();
}

hipError_t launch_member_bytes(const uint32_t *ids, uint64_t n_pos, uint64_t n_rows, uint8_t *member, uint32_t *bad, hipStream_t s) {
    if (n_pos == 0) return hipSuccess;
    if (!ids || !bad || (n_rows && !member) || n_pos > (1ull << 32)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(member_bytes_kernel, dim3((uint32_t)quads_blocks(n_pos)), dim3(256), 0, s, ids, n_pos, n_rows, member, bad);
    return hipGetLastError();
}

hipError_t launch_lists_remap(const uint32_t *ids, uint64_t n_pos, const uint64_t *rowbits, uint64_t n_rows, const uint64_t *rank,
                              uint32_t *out, hipStream_t s) {
    if (n_pos == 0) return hipSuccess;
    if (!ids || !rowbits || !rank || !out || n_pos > (1ull << 32) || (reinterpret_cast<uintptr_t>(out) & 15u) != 0) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lists_remap_kernel, dim3((uint32_t)quads_blocks(n_pos)), dim3(256), 0, s, ids, n_pos, rowbits, n_rows, rank, out);
    return hipGetLastError();
}

hipError_t launch_rows_gather(const float *src, const uint32_t *old_row, uint64_t m, uint32_t dim, float *dst, hipStream_t s) {
    if (m == 0 || dim == 0) return hipSuccess;
    if (!src || !old_row || !dst || dim > (1u << 30)) return hipErrorInvalidValue;
    const bool wide = (dim % 4) == 0 && ((reinterpret_cast<uintptr_t>(src) | reinterpret_cast<uintptr_t>(dst)) & 15u) == 0;
    const uint32_t g = wide ? dim / 4 : dim;
    const uint64_t blocks = (m * g + 1023) / 1024;
    if (blocks > 0x7FFFFFFFull) return hipErrorInvalidValue;
    if (wide)
        hipLaunchKernelGGL(rows_gather_kernel<f32x4>, dim3((uint32_t)blocks), dim3(256), 0, s, reinterpret_cast<const f32x4 *>(src), old_row, m, g,
                           reinterpret_cast<f32x4 *>(dst));
    else
        hipLaunchKernelGGL(rows_gather_kernel<float>, dim3((uint32_t)blocks), dim3(256), 0, s, src, old_row, m, g, dst);
    return hipGetLastError();
}

}  // namespace pqv
