// kernels_grouped.hip -- gfx950 kernels of the grouped top-k (pqv.h: pqv_topk_grouped): up to group_size rows of each of the k
// nearest groups.  The call is two passes over the same candidates.  Pass 1 is the distinct call as it stands (kernels_distinct.hip)
// and names the k groups; everything here is pass 2, which knows a row's group before it reads the row:
//
//   group_set_kernel        the first n_found group values of a query, sorted ascending, each with its rank in pass 1 (its SLOT)
//   WaveGroupedTopk<S>      a wave-distributed list ascending by (slot, key) that holds at most group_size entries per slot
//   grouped_stream_kernel   distinct_stream_kernel's exact walk over the positions whose group value is in the query's set
//   grouped_merge_kernel    one wave per query folds the per-wave partial lists through the same offer and writes [q][slot][i]
//
// Why no one-pass list: with several rows per group a row refused because its group is not among the k nearest NOW may be the
// second best of a group that a later, nearer row pulls in, and a kept row of a near group can have any number of rows of other
// groups in front of it -- no bounded (d2, position) list is exact.  With the groups fixed, every slot is an independent
// "group_size smallest keys" selection, and the list below is k of those side by side.
//
// The invariant (tests/test_grouped_host.py models it): after any sequence of offers, slot g's entries are the min(group_size,
// offered) smallest keys offered for g.  An offer inserts while g holds fewer than group_size entries, else replaces g's largest
// entry if the candidate is smaller; neither touches another slot's set.  Only members of the k groups are offered, so the list
// holds at most k * group_size <= S * 64 entries: it cannot overflow and needs no admission threshold.
//
// The fold is exact for the plain reason: each of slot g's global group_size smallest keys is among the group_size smallest of
// the partition that holds it, so it reaches the fold, where the same offer keeps the smallest per slot.
#include "stream_walk.hpp"
#include "wave_group_lists.hpp"

namespace pqv {

// GROUPED_SLOT_EMPTY, WaveGroupedTopk<S>: wave_group_lists.hpp

// ------------------------------------------------------------------------------------
// group_set_kernel: one block per query.  Reads the first n_found[q] group values of pass 1 -- never the padding behind them, whose 0
// may be a real group -- and writes them ascending (rank counting in LDS: the values are distinct) with each value's slot, its
// rank in pass 1, to set_keys / set_slot [nq][k].  k <= GROUPED_SET_MAX.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_set_kernel(const int64_t *group_key, const uint32_t *n_found, uint32_t k, int64_t *set_keys,
                                                        uint32_t *set_slot) {
    __shared__ int64_t vals[GROUPED_SET_MAX];
    const uint32_t q = blockIdx.x;
    uint32_t n = n_found[q];
    if (n > k) n = k;
    const uint64_t base = (uint64_t)q * k;
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) vals[i] = group_key[base + i];
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += blockDim.x) {
        const int64_t v = vals[i];
        uint32_t rank = 0;
        for (uint32_t j = 0; j < n; ++j) rank += vals[j] < v ? 1u : 0u;
        set_keys[base + rank] = v;
        set_slot[base + rank] = i;
    }
}

hipError_t launch_group_set(const int64_t *group_key, const uint32_t *n_found, uint32_t nq, uint32_t k, int64_t *set_keys, uint32_t *set_slot,
                            hipStream_t s) {
    if (!group_key || !n_found || !set_keys || !set_slot || k == 0 || k > GROUPED_SET_MAX) return hipErrorInvalidValue;
    if (nq == 0) return hipSuccess;
    hipLaunchKernelGGL(group_set_kernel, dim3(nq), dim3(256), 0, s, group_key, n_found, k, set_keys, set_slot);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// grouped_stream_kernel
//
// distinct_stream_kernel's walk, composed of the same pieces (stream_walk.hpp): its grid (row block, probe rank, query), its 4
// independent waves per block, its clamped walk range, its filtered walk and its chain tile -- so a row's d2 has the bits pass 1
// gave it -- and its keys.  A window's 64 bits
// are the AND of three sources: the group column's validity image, the shared mask's image, and MEMBERSHIP -- lane l reads
// key_pos[p + l] (one coalesced window, as the keyed kernel reads it), sign-extends an i32 value, and looks it up in the query's
// sorted set by a branch-free binary search over full i64 values.  The set (5 KB: GROUPED_SET_MAX i64 values and u16 slots) is
// staged once per block in LDS beside the tile area.  A row outside the k groups is never read.  The slot found by the lookup
// travels through the queue beside the list offset, and lane l offers (key, storage row, slot) to a WaveGroupedTopk.
//
// The wave writes the filled part of its list to part_keys / part_vals / part_slot [nq][n_part][km] and the length to part_cnt
// [nq][n_part]: most waves of a call meet a handful of members, and the fold reads what was written, not km entries per wave.
// Statistics: the rows evaluated here are added to the embeddings_fetched word; candidate_rows was counted by pass 1.
// ------------------------------------------------------------------------------------
template <int CG, int S, bool SEQ, bool ALIGNED, int GW>
__global__ __launch_bounds__(256) void grouped_stream_kernel(const StreamArgs a, const GroupedArgs ga) {
    static_assert(tile_words<CG, SEQ>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words<CG, SEQ>()];
    __shared__ int64_t set_v[GROUPED_SET_MAX];
    __shared__ uint16_t set_s[GROUPED_SET_MAX];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words<CG, SEQ>();

    const uint32_t q = blockIdx.z, j = blockIdx.y;
    // a rank at or beyond the query's limit (pqv_topk_grouped_expand) walks nothing (block-uniform: nobody is left at the barrier)
    if (ga.rank_limit && j >= ga.rank_limit[q]) {
        if (lane == 0) ga.part_cnt[partial_base(a, q, j, wave, 1)] = 0;
        return;
    }
    // the query's set (block-uniform; every wave of the block passes the barrier before it looks at its range)
    GroupSet gs;
    gs.stage(ga, q, set_v, set_s);
    __syncthreads();

    WalkRange w = walk_range<true>(a, q, j, wave);
    if (gs.n == 0) w.r1 = 0;            // no group: nothing to walk, an empty list is written
    unsigned long long *st = stats_slot(ga.stats, q);

    const float *qv = a.queries + (uint64_t)q * a.dim;
    WaveGroupedTopk<S> tk;
    tk.init();

    const uint32_t n_eval = filtered_walk<true>(
        w.lbeg, w.r0, w.r1, lds, lane,
        [&](uint64_t p, uint64_t, uint64_t clip, uint32_t &slot) {
            const uint64_t win = group_images_window(ga.valid_pos, ga.bits, p, clip);
            if (win == 0) return win;
            return win & group_member_window(gs, ga.key_pos, GW == 1, p, lane, slot);
        },
        [&](const QueueTile &t) { grouped_tile<CG, SEQ, ALIGNED>(a, ga.group_size, w, t, lds, qv, lane, tk); });
    if (st && n_eval && lane == 0) atomicAdd(&st[3], (unsigned long long)n_eval);
    write_grouped_lists<S>(a, ga, q, j, wave, lane, tk);
}

template <int S, int GW>
static hipError_t launch_grouped_s(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    return dispatch_chunk(a.dim, a.metric, [&](auto cg, auto seq, auto aligned) {
        dim3 grid(a.blocks_per_list, a.nprobe, a.nq);
        hipLaunchKernelGGL((grouped_stream_kernel<cg.value, S, seq.value, aligned.value, GW>), grid, dim3(256), 0, s, a, ga);
        return hipGetLastError();
    });
}

template <int GW>
static hipError_t launch_grouped_w(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    return dispatch_list_slots(ga.km, [&](auto S) { return launch_grouped_s<S.value, GW>(a, ga, s); });     // (km <= 1024: grouped_shape_ok)
}

// k * group_size <= 1024 with group_size >= 2 (one row per group is the distinct call), hence k <= GROUPED_SET_MAX
static bool grouped_shape_ok(uint32_t k, uint32_t group_size, uint32_t km) {
    return k != 0 && group_size >= 2 && (uint64_t)k * group_size == km && km <= 1024 && k <= GROUPED_SET_MAX;
}

hipError_t launch_grouped_stream(const StreamArgs &a, const GroupedArgs &ga, hipStream_t s) {
    if (!a.probe || !a.list_off || !a.cand_base || !ga.part_keys || !ga.part_vals || !ga.part_slot || !ga.part_cnt) return hipErrorInvalidValue;
    if (!ga.key_pos || !ga.set_keys || !ga.set_slot || !ga.n_found || !grouped_shape_ok(ga.k, ga.group_size, ga.km)) return hipErrorInvalidValue;
    if (a.nq == 0 || a.blocks_per_list == 0 || a.nprobe == 0) return hipSuccess;
    if (ga.elem_size == 4) return launch_grouped_w<1>(a, ga, s);
    if (ga.elem_size == 8) return launch_grouped_w<2>(a, ga, s);
    return hipErrorInvalidValue;
}

// ------------------------------------------------------------------------------------
// grouped_merge_kernel: one wave per query folds the query's n_part partial lists through WaveGroupedTopk::offer -- the lengths
// of 64 lists per load, then 64 entries of a list per step, only the filled ones.  The folded list is ascending by (slot, key), so
// the write-out is a segmented index: the list goes to LDS, the first entry of a segment records the segment's start and the
// last one its length, and output (g, i) is entry start[g] + i where i < rows[g], else the padding (0xFFFFFFFF, +inf).  Storage
// row -> reported row through ids, sqrt (IEEE) or the cosine halving as the distinct fold applies them.  group_rows[q][g] = rows[g]
// (0 for a slot with no group).  group_key and n_found are pass 1's.
// ------------------------------------------------------------------------------------
template <int S>
__global__ __launch_bounds__(64) void grouped_merge_kernel(const GroupedMergeArgs a) {
    __shared__ uint64_t l_key[S * 64];
    __shared__ uint32_t l_val[S * 64];
    __shared__ uint32_t l_start[GROUPED_SET_MAX];
    __shared__ uint32_t l_rows[GROUPED_SET_MAX];
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const uint32_t k = a.k, m = a.group_size, km = a.km;
    WaveGroupedTopk<S> tk;
    tk.init();

    for (uint32_t p0 = 0; p0 < a.n_part; p0 += 64) {
        const uint32_t pl = p0 + (uint32_t)lane;
        uint32_t mycnt = pl < a.n_part ? a.part_cnt[(uint64_t)q * a.n_part + pl] : 0u;
        if (mycnt > km) mycnt = km;
        unsigned long long todo = __ballot(mycnt != 0);
        while (todo) {
            const int L = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint32_t cnt = readlane_u32(mycnt, L);
            const uint64_t base = ((uint64_t)q * a.n_part + p0 + (uint32_t)L) * km;
            for (uint32_t e0 = 0; e0 < cnt; e0 += 64) {
                const uint32_t e = e0 + (uint32_t)lane;
                const bool in = e < cnt;
                const uint64_t kv = in ? a.part_keys[base + e] : KEY_EMPTY;
                const uint32_t vv = in ? a.part_vals[base + e] : 0xFFFFFFFFu;
                const uint32_t sv = in ? a.part_slot[base + e] : 0u;
                // (a slot at or beyond k cannot come from the stream kernel; kept out so that no index below leaves its array)
                tk.offer(in && sv < k ? kv : KEY_EMPTY, vv, sv, m, lane);
            }
        }
    }

    for (uint32_t g = lane; g < k; g += 64) l_rows[g] = 0;
    wave_lds_fence();
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        l_key[e] = tk.key[s];
        l_val[e] = tk.val[s];
        // the slot of element e - 1 (lane 0: the last lane of the register below; element 0: none)
        uint32_t prev = (uint32_t)__shfl_up((int)tk.slot[s], 1, 64);
        const uint32_t below = s > 0 ? readlane_u32(tk.slot[s > 0 ? s - 1 : 0], 63) : GROUPED_SLOT_EMPTY;
        if (lane == 0) prev = below;
        const uint32_t mine = tk.slot[s];
        if (e < tk.n && prev != mine) l_start[mine] = e;
    }
    wave_lds_fence();
#pragma unroll
    for (int s = 0; s < S; ++s) {
        const uint32_t e = s * 64 + lane;
        // the slot of element e + 1 (lane 63: the first lane of the register above; the last element: none)
        uint32_t next = (uint32_t)__shfl_down((int)tk.slot[s], 1, 64);
        const uint32_t above = s + 1 < S ? readlane_u32(tk.slot[s + 1 < S ? s + 1 : s], 0) : GROUPED_SLOT_EMPTY;
        if (lane == 63) next = above;
        const uint32_t mine = tk.slot[s];
        if (e < tk.n && next != mine) l_rows[mine] = e + 1 - l_start[mine];
    }
    wave_lds_fence();

    const uint64_t obase = (uint64_t)q * km;
    for (uint32_t o = lane; o < km; o += 64) {
        const uint32_t g = o / m, i = o - g * m;
        uint32_t row = 0xFFFFFFFFu;
        float d = INFINITY;
        if (i < l_rows[g]) {
            const uint32_t e = l_start[g] + i;
            const float d2 = __uint_as_float((uint32_t)(l_key[e] >> 32));
            row = a.ids ? a.ids[l_val[e]] : l_val[e];
            d = a.sqrt_out == 1 ? sqrt_f32_ieee(d2) : a.sqrt_out == 2 ? 0.5f * d2 : d2;
        }
        a.row_idx[obase + o] = row;
        a.dist[obase + o] = d;
    }
    if (a.group_rows)
        for (uint32_t g = lane; g < k; g += 64) a.group_rows[(uint64_t)q * k + g] = l_rows[g];
}

hipError_t launch_grouped_merge(const GroupedMergeArgs &a, hipStream_t s) {
    if (!a.part_keys || !a.part_vals || !a.part_slot || !a.part_cnt || !a.row_idx || !a.dist) return hipErrorInvalidValue;
    if (!grouped_shape_ok(a.k, a.group_size, a.km)) return hipErrorInvalidValue;
    if (a.nq == 0) return hipSuccess;
    const dim3 grid(a.nq), block(64);
    return dispatch_list_slots(a.km, [&](auto S) {
        hipLaunchKernelGGL((grouped_merge_kernel<S.value>), grid, block, 0, s, a);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------------------------
// group_rows_fill_kernel: group_size == 1 takes the distinct call as it stands, whose groups have one row each:
// group_rows[q][g] = g < n_found[q].
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void group_rows_fill_kernel(const uint32_t *n_found, uint32_t nq, uint32_t k, uint32_t *group_rows) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (uint64_t)nq * k) return;
    group_rows[i] = (uint32_t)(i % k) < n_found[i / k] ? 1u : 0u;
}

hipError_t launch_group_rows_fill(const uint32_t *n_found, uint32_t nq, uint32_t k, uint32_t *group_rows, hipStream_t s) {
    if (!n_found || !group_rows || k == 0) return hipErrorInvalidValue;
    if (nq == 0) return hipSuccess;
    const uint64_t n = (uint64_t)nq * k;
    hipLaunchKernelGGL(group_rows_fill_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s, n_found, nq, k, group_rows);
    return hipGetLastError();
}

}  // namespace pqv
