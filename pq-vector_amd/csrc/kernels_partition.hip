// kernels_partition.hip -- gfx950 kernels of the key partitions (pqv.h: pqv_key_partition): a second set of lists over a searcher's
// rows, keyed by a filter column instead of the centroids.  A partition holds the searcher's LIST POSITIONS whose row has a valid key,
// sorted by (key as i64, row id), the distinct key values ascending and the first entry of every value's run.
//   build                    partition_gather_kernel, partition_keys_kernel and partition_off_kernel around two stable radix sorts, a
//                            run-length pass and a scan -- rocPRIM's, header-only from the ROCm tree (kernels.h has the order)
//   partition_span_kernel    a query's filter (PQV_KEY_EQ / RANGE / IN) -> spans of the partition: lower / upper bound searches in
//                            the distinct-value table, for IN one per slice value and the prefix sums of the span lengths
//   partition_stream_kernel  the exact distance pass over a query's candidate sequence: masked_stream_kernel's tile and list over
//                            PartitionSeq's walk (stream_walk.hpp), a grid that does not depend on the span lengths
// Nothing is probed: with no mask the answer is the exact top-k over ALL indexed rows whose key passes.
#include "stream_walk.hpp"

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_run_length_encode.hpp>
#include <rocprim/device/device_scan.hpp>

namespace pqv {

// ------------------------------------------------------------------------------------
// build
// ------------------------------------------------------------------------------------
// row_key[p] = the row list position p reports (ids[p]) where it is a row of the column with a valid key, else 0xFFFFFFFF (no row
// has that id: a corpus holds at most 2^32 - 1 rows); pos[p] = p.  The positions with a key: a popcount and one atomicAdd per wave.
__global__ __launch_bounds__(256) void partition_gather_kernel(const uint8_t *valid, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos,
                                                               uint32_t *row_key, uint32_t *pos, unsigned long long *count) {
    const uint64_t p = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    bool on = false;
    if (p < n_pos) {
        const uint64_t r = ids ? ids[p] : p;
        on = r < n_rows && r < 0xFFFFFFFFull && (!valid || valid[r] != 0);
        row_key[p] = on ? (uint32_t)r : 0xFFFFFFFFu;
        pos[p] = (uint32_t)p;
    }
    const uint64_t m = __ballot(on);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count, (unsigned long long)__popcll(m));
}

// key[i] = values[row_key[i]], an i32 column's value widened (T: int32_t / int64_t), i < m
template <class T>
__global__ __launch_bounds__(256) void partition_keys_kernel(const T *values, const uint32_t *row_key, uint64_t m, int64_t *key) {
    const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < m) key[i] = (int64_t)values[row_key[i]];
}

// key_off[n_keys] = m, behind the exclusive scan that wrote key_off[0 .. n_keys) (n_keys is on the device only)
__global__ void partition_off_kernel(const unsigned long long *n_keys, uint64_t m, uint64_t *key_off) { key_off[*n_keys] = m; }

static inline hipError_t grid_256(uint64_t n, uint32_t *blocks) {
    const uint64_t b = (n + 255) / 256;
    if (b > 0x7FFFFFFFull) return hipErrorInvalidValue;
    *blocks = (uint32_t)b;
    return hipSuccess;
}

hipError_t launch_partition_tmp_bytes(uint64_t n_pos, size_t *bytes) {
    size_t b = 0, most = 0;
    const size_t n = (size_t)n_pos;
    hipError_t e = rocprim::radix_sort_pairs(nullptr, b, (const uint32_t *)nullptr, (uint32_t *)nullptr, (const uint32_t *)nullptr,
                                             (uint32_t *)nullptr, n, 0, 32, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
    e = rocprim::radix_sort_pairs(nullptr, b, (const int64_t *)nullptr, (int64_t *)nullptr, (const uint32_t *)nullptr, (uint32_t *)nullptr, n,
                                  0, 64, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
    e = rocprim::run_length_encode(nullptr, b, (const int64_t *)nullptr, n, (int64_t *)nullptr, (uint64_t *)nullptr,
                                   (unsigned long long *)nullptr, (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
    e = rocprim::exclusive_scan(nullptr, b, (const uint64_t *)nullptr, (uint64_t *)nullptr, (uint64_t)0, n, rocprim::plus<uint64_t>(),
                                (hipStream_t) nullptr);
    if (e != hipSuccess) return e;
    most = b > most ? b : most;
    *bytes = most;
    return hipSuccess;
}

hipError_t launch_partition_gather(const uint8_t *valid, uint64_t n_rows, const uint32_t *ids, uint64_t n_pos, uint32_t *row_key, uint32_t *pos,
                                   unsigned long long *count, hipStream_t s) {
    if (n_pos == 0) return hipSuccess;
    if (n_pos > 0xFFFFFFFFull) return hipErrorInvalidValue;
    uint32_t blocks = 0;
    if (hipError_t e = grid_256(n_pos, &blocks)) return e;
    hipLaunchKernelGGL(partition_gather_kernel, dim3(blocks), dim3(256), 0, s, valid, n_rows, ids, n_pos, row_key, pos, count);
    return hipGetLastError();
}

hipError_t launch_partition_sort_rows(const uint32_t *row_key, const uint32_t *pos, uint32_t *row_key_out, uint32_t *pos_out, uint64_t n_pos,
                                      void *tmp, size_t tmp_bytes, hipStream_t s) {
    if (n_pos == 0) return hipSuccess;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, row_key, row_key_out, pos, pos_out, (size_t)n_pos, 0, 32, s);
}

hipError_t launch_partition_keys(const void *values, uint32_t elem_size, const uint32_t *row_key, uint64_t m, int64_t *key, hipStream_t s) {
    if (elem_size != 4 && elem_size != 8) return hipErrorInvalidValue;
    if (m == 0) return hipSuccess;
    uint32_t blocks = 0;
    if (hipError_t e = grid_256(m, &blocks)) return e;
    if (elem_size == 4)
        hipLaunchKernelGGL(partition_keys_kernel<int32_t>, dim3(blocks), dim3(256), 0, s, static_cast<const int32_t *>(values), row_key, m, key);
    else
        hipLaunchKernelGGL(partition_keys_kernel<int64_t>, dim3(blocks), dim3(256), 0, s, static_cast<const int64_t *>(values), row_key, m, key);
    return hipGetLastError();
}

hipError_t launch_partition_sort_keys(const int64_t *key, const uint32_t *pos, int64_t *key_out, uint32_t *pos_out, uint64_t m, void *tmp,
                                      size_t tmp_bytes, hipStream_t s) {
    if (m == 0) return hipSuccess;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, key, key_out, pos, pos_out, (size_t)m, 0, 64, s);
}

hipError_t launch_partition_runs(const int64_t *key, uint64_t m, int64_t *keys, uint64_t *cnt, uint64_t *key_off, unsigned long long *n_keys,
                                 void *tmp, size_t tmp_bytes, hipStream_t s) {
    if (m == 0) return hipSuccess;      // (the caller has zeroed *n_keys and key_off[0])
    size_t b = tmp_bytes;
    hipError_t e = rocprim::run_length_encode(tmp, b, key, (size_t)m, keys, cnt, n_keys, s);
    if (e != hipSuccess) return e;
    // (over all m slots: the lengths behind the n_keys-th are not read again, and key_off[n_keys] is set below)
    b = tmp_bytes;
    e = rocprim::exclusive_scan(tmp, b, cnt, key_off, (uint64_t)0, (size_t)m, rocprim::plus<uint64_t>(), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(partition_off_kernel, dim3(1), dim3(1), 0, s, n_keys, m, key_off);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// partition_span_kernel
//
// KIND 0 / 1 (PQV_KEY_EQ / PQV_KEY_RANGE): one thread per query, two bound searches in the distinct-value table: the span is
// [key_off[first value >= lo], key_off[first value > hi]), empty for lo > hi.  KIND 2 (PQV_KEY_IN): one block per query, thread t
// looks up the slice values 4 t .. 4 t + 3 (a value that is no key of the partition gives an empty span: an I32 partition's table
// holds widened i32 values only, so a value outside i32 is simply absent); wave 0 then turns the lengths into inclusive prefix sums,
// saturated at 2^32 - 1.  n = min(lims[q + 1] - lims[q], KEY_SET_MAX) values are read, none for an inverted slice: every index
// into the outputs is below KEY_SET_MAX per query whatever the slice holds.
// ------------------------------------------------------------------------------------
// the first index in [0, n) whose key is >= v (UPPER: > v), n where there is none
template <bool UPPER>
__device__ __forceinline__ uint64_t partition_bound(const int64_t *keys, uint64_t n, int64_t v) {
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = lo + ((hi - lo) >> 1);
        const int64_t kv = keys[mid];
        if (UPPER ? kv <= v : kv < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ uint64_t shfl_up_u64(uint64_t v, int d) {
    const uint32_t lo = (uint32_t)__shfl_up((int)(uint32_t)v, d, 64);
    const uint32_t hi = (uint32_t)__shfl_up((int)(uint32_t)(v >> 32), d, 64);
    return ((uint64_t)hi << 32) | lo;
}

template <int KIND>
__global__ __launch_bounds__(256) void partition_span_kernel(const PartitionSpanArgs a) {
    constexpr uint64_t SEQ_MAX = 0xFFFFFFFFull;
    if constexpr (KIND != 2) {
        const uint32_t q = blockIdx.x * 256 + threadIdx.x;
        if (q >= a.nq) return;
        const int64_t lo = static_cast<const int64_t *>(a.a)[q];
        const int64_t hi = KIND == 0 ? lo : static_cast<const int64_t *>(a.b)[q];
        uint64_t beg = 0, len = 0;
        if (lo <= hi && a.n_keys) {
            const uint64_t j0 = partition_bound<false>(a.keys, a.n_keys, lo), j1 = partition_bound<true>(a.keys, a.n_keys, hi);
            if (j1 > j0) { beg = a.key_off[j0]; len = a.key_off[j1] - beg; }
        }
        if (len > SEQ_MAX) len = SEQ_MAX;
        a.span_beg[q] = (uint32_t)beg;
        a.n_cand[q] = len;
        if (a.n_cand_out) a.n_cand_out[q] = len;
        unsigned long long *st = stats_slot(a.stats, q);
        if (st && len) atomicAdd(&st[2], (unsigned long long)len);
    } else {
        __shared__ uint32_t s_len[KEY_SET_MAX];
        const uint32_t q = blockIdx.x;
        const uint64_t s0 = static_cast<const uint64_t *>(a.a)[q], s1 = static_cast<const uint64_t *>(a.a)[q + 1];
        uint32_t n = 0;
        if (s1 > s0) n = s1 - s0 > (uint64_t)KEY_SET_MAX ? KEY_SET_MAX : (uint32_t)(s1 - s0);
        const uint64_t ob = (uint64_t)q * KEY_SET_MAX;
        for (uint32_t i = threadIdx.x; i < KEY_SET_MAX; i += 256) {
            uint64_t beg = 0, len = 0;
            if (i < n && a.n_keys) {
                const int64_t v = static_cast<const int64_t *>(a.b)[s0 + i];
                const uint64_t j = partition_bound<false>(a.keys, a.n_keys, v);
                if (j < a.n_keys && a.keys[j] == v) { beg = a.key_off[j]; len = a.key_off[j + 1] - beg; }
            }
            s_len[i] = (uint32_t)len;       // (a run is shorter than 2^32: m is)
            if (i < n) a.span_beg[ob + i] = (uint32_t)beg;
        }
        __syncthreads();
        if (threadIdx.x < 64) {
            // lane l owns the 16 values from 16 l on: their sum, an inclusive scan over the lanes, then the running sums
            const int lane = threadIdx.x;
            uint64_t own = 0;
            for (int u = 0; u < 16; ++u) own += s_len[lane * 16 + u];
            uint64_t incl = own;
            for (int d = 1; d < 64; d <<= 1) {
                const uint64_t o = shfl_up_u64(incl, d);
                if (lane >= d) incl += o;
            }
            uint64_t run = incl - own;
            for (int u = 0; u < 16; ++u) {
                const uint32_t i = lane * 16 + u;
                run += s_len[i];
                if (i < n) a.span_end[ob + i] = (uint32_t)(run > SEQ_MAX ? SEQ_MAX : run);
            }
            if (lane == 63) {
                const uint64_t total = run > SEQ_MAX ? SEQ_MAX : run;
                a.n_span[q] = n;
                a.n_cand[q] = total;
                if (a.n_cand_out) a.n_cand_out[q] = total;
                unsigned long long *st = stats_slot(a.stats, q);
                if (st && total) atomicAdd(&st[2], (unsigned long long)total);
            }
        }
    }
}

hipError_t launch_partition_span(const PartitionSpanArgs &a, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!a.a || !a.span_beg || !a.n_cand || (a.n_keys && (!a.keys || !a.key_off))) return hipErrorInvalidValue;
    if (a.kind == 0) {
        hipLaunchKernelGGL(partition_span_kernel<0>, dim3((a.nq + 255) / 256), dim3(256), 0, s, a);
    } else if (a.kind == 1) {
        if (!a.b) return hipErrorInvalidValue;
        hipLaunchKernelGGL(partition_span_kernel<1>, dim3((a.nq + 255) / 256), dim3(256), 0, s, a);
    } else if (a.kind == 2) {
        if (!a.b || !a.span_end || !a.n_span) return hipErrorInvalidValue;
        hipLaunchKernelGGL(partition_span_kernel<2>, dim3(a.nq), dim3(256), 0, s, a);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// partition_stream_kernel
//
// grid = (B, nq); block = 256 threads = 4 independent waves with masked_stream_kernel's tile area and nothing beside it.  The
// query's sequence has n_cand[q] positions, known on the device only, so the grid cannot follow it: wave w of block x takes the
// 64-position windows (turn * B + x) * 4 + w for turn = 0, 1, ... while they begin inside the sequence (PartitionSeq,
// stream_walk.hpp: the distinct / grouped passes of kernels_partition_group.hip and the range pass walk the same way).  A window's
// position `seq` is mapped to its partition entry -- one span (EQ / RANGE): span_beg[q] + seq; IN: the first span whose inclusive prefix
// sum exceeds seq, found by a halving search over the query's n_span[q] <= KEY_SET_MAX sums (read through the caches: no LDS
// beside the tile, the occupancy of the masked twin) -- and the entry's list position is loaded: one coalesced 256-byte read per
// span a window touches.
// MASKED = false: the window IS the tile (PartitionSeq::windows).  MASKED: PartitionSeq::filtered_windows under image_bit of the
// mask's image -- the set positions are compacted through a WindowQueue, each with its list position as payload; a tile runs
// whenever 64 are queued and once more behind the wave's last window, from ONE call site, so a row the mask excludes is never
// loaded and the list's offer is instantiated once (the 1024-entry lists stay in registers).  Sequence positions stay the unmasked
// ones.
// Keys: (d2 bits << 32) | seq (l2_key) or (ord(dist) << 32) | seq (dot_key); storage rows through storage_row.  The per-wave lists
// go out in StreamArgs' format (nprobe = 1, blocks_per_list = B) for merge_kernel / dot_merge_kernel; a wave without a window
// writes its EMPTY list.  One statistics add per wave: the rows evaluated, to embeddings_fetched.
// ------------------------------------------------------------------------------------
// (CG 32's tile area lets 5 blocks share a CU: the masked forms of the lists up to 256 entries are held to 5 waves' registers)
template <int CG, int S, bool SEQ, bool ALIGNED, bool DOT, bool MASKED>
__global__ __launch_bounds__(256, (MASKED && CG == 32 && S <= 4) ? 5 : 1) void partition_stream_kernel(const StreamArgs a, const PartitionArgs pa) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.y;
    PartitionSeq ps;
    ps.setup(pa, q);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveTopk<S> tk;
    tk.init();
    uint32_t n_eval = 0;

    // a tile of nvalid rows: lane l holds list position lpos at sequence position seq (both clamped to the tile's last row)
    auto tile = [&](uint32_t lpos, uint32_t seq, uint32_t nvalid) {
        const uint32_t my_srow = storage_row(a, lpos);
        float sum;
        if constexpr (DOT) sum = dot_tile<CG, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
        else sum = l2_tile<CG, SEQ, ALIGNED>(a, lds, qv, my_srow, nvalid, lane);
        const bool valid = (uint32_t)lane < nvalid;
        const uint64_t key = DOT ? dot_key(sum, seq) : l2_key(sum, seq);
        tk.offer(valid ? key : KEY_EMPTY, my_srow, a.k, lane);
        n_eval += nvalid;
    };

    if constexpr (!MASKED) {
        ps.windows(ps.total, wave, lane, [&](uint64_t, uint32_t nvalid, uint32_t seq, uint32_t lpos) { tile(lpos, seq, nvalid); });
    } else {
        ps.filtered_windows(ps.total, lds, wave, lane, [&](uint32_t lpos) { return image_bit(pa.bits, lpos); }, tile);
    }
    unsigned long long *st = stats_slot(pa.stats, q);
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);

    write_partial_lists<S>(a.part_keys, a.part_vals, partial_base(a, q, 0, wave, a.k), a.k, lane, tk.key, tk.val);
}

template <int S, bool DOT, bool MASKED>
static hipError_t launch_partition_s(const StreamArgs &a, const PartitionArgs &pa, hipStream_t s) {
    return dispatch_chunk<!DOT>(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nq);
        hipLaunchKernelGGL((partition_stream_kernel<cg.value, S, seq.value, aligned.value, DOT, MASKED>), grid, dim3(256), 0, s, a, pa);
        return hipGetLastError();
    });
}

hipError_t launch_partition_stream(const StreamArgs &a, const PartitionArgs &pa, hipStream_t s) {
    if (a.nq == 0) return hipSuccess;
    if (!partition_walk_ok(a, pa) || !a.part_keys || !a.part_vals) return hipErrorInvalidValue;
    const bool dot = a.metric == 4;     // PQV_DOT
    return dispatch_list_slots(a.k, [&](auto S) {
        if (dot) return pa.bits ? launch_partition_s<S.value, true, true>(a, pa, s) : launch_partition_s<S.value, true, false>(a, pa, s);
        return pa.bits ? launch_partition_s<S.value, false, true>(a, pa, s) : launch_partition_s<S.value, false, false>(a, pa, s);
    });
}

}  // namespace pqv
