// kernels_group_expand.hip -- the gfx950 kernel of the expanding distinct / grouped top-k (pqv.h: pqv_topk_distinct_expand,
// pqv_topk_grouped_expand): group_expand_kernel decides, per query, how many of its P probed lists hold k DISTINCT group values
// among the rows the call's stream pass would walk.  distinct_stream_kernel, grouped_stream_kernel and their filtered forms then
// walk each query's lists below its own rank limit (DistinctArgs / GroupedArgs::rank_limit).  No embedding is read here.
//
// Rows cannot be counted per list and summed (kernels_expand.hip): ten passing rows of two lists may be ten chunks of one document.
// What is counted is the SIZE OF A SET, so the kernel keeps the set: one block per query, an open-addressed hash set of i64 group
// values in LDS, filled in probe order.
//
// Why the result is exact and does not depend on the order in which waves insert:
//   * a value enters the set through one atomicCAS on one slot of its probe sequence; of all lanes that offer the same value
//     exactly one sees the slot EMPTY, every other sees the value -- whichever lane wins, the set's size grows by one per value;
//   * the probe sequence (home slot from a multiplicative hash, then linear, GROUP_SET_SLOTS steps at most) visits every slot, and
//     the set never fills: a wave starts a window only while the counter is below k and adds at most 64 values before it
//     counts them, so at most k - 1 + 4 * 64 <= 1279 of the 4096 slots are ever taken.  Values with the same home slot -- or
//     congruent modulo the table size -- just probe further; full 64-bit values are compared, never hashes;
//   * the one value that equals the EMPTY marker (-1) never enters the table: a flag of its own counts it once;
//   * the decision is taken after COMPLETE ranks only, between two block barriers: is the set's size >= k.  A wave that sees the
//     counter at k inside a list stops inserting -- the count after the whole list could only be larger, and every earlier rank was
//     counted completely, so the first rank at which the decision is "yes" is the same with or without the early stop.
#include "stream_walk.hpp"

namespace pqv {

// one value into the set; true: this lane added it (it was not there)
__device__ __forceinline__ bool group_set_insert(unsigned long long *tab, uint32_t *marker_seen, uint64_t v) {
    if (v == GROUP_SET_EMPTY) return atomicExch(marker_seen, 1u) == 0u;
    const uint32_t h = group_set_home(v);
    for (uint32_t i = 0; i < GROUP_SET_SLOTS; ++i) {
        const uint32_t at = (h + i) & (GROUP_SET_SLOTS - 1u);
        const unsigned long long old = atomicCAS(&tab[at], (unsigned long long)GROUP_SET_EMPTY, (unsigned long long)v);
        if (old == GROUP_SET_EMPTY) return true;
        if (old == v) return false;
    }
    return false;       // (a full table: cannot be, see above)
}

// ------------------------------------------------------------------------------------
// group_expand_kernel<FK, GW>: grid (query), 256 threads.  FK 0: no per-query filter; 1: PQV_KEY_EQ / PQV_KEY_RANGE (one test, as
// the filtered stream kernels run it); 2: PQV_KEY_IN (the slice staged once through setup_in).  GW: the group column's width in
// words.  The block walks the query's probe ranks 0 .. P - 1 in order; a list is walked in 64-position windows at multiples of 64
// from its start, clipped at its end -- the windows of filter_count_kernel and of the stream kernels -- the four waves striding over
// them.  A window's bits are the stream twins': group_images_window ANDed with KeyTest::window.  Lanes whose bit is set load their
// group value and insert it; a wave that added values bumps the LDS counter by their number.  A window without a set bit loads no
// group key.  After each rank all waves agree (two barriers around one read) whether the counter has reached k: the first rank j at
// which it has gives used = max(p0, j + 1), else used = P.  An empty IN slice walks nothing.
// Thread 0 writes nprobe_used[q] = used and OVERWRITES n_cand[q] exactly as expand_select_kernel does.
// probe / list_off / cand_base words are block-uniform and read with uniform_word: the trip counts below are scalar.
// ------------------------------------------------------------------------------------
template <int FK, int GW>
__global__ __launch_bounds__(256) void group_expand_kernel(const GroupExpandArgs a, const GroupFilterArgs fa) {
    __shared__ unsigned long long tab[GROUP_SET_SLOTS];
    __shared__ uint32_t s_count, s_marker;
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const uint32_t q = blockIdx.x;

    KeyTest<FK == 2 ? 2 : 1> kt;
    for (uint32_t i = threadIdx.x; i < GROUP_SET_SLOTS; i += 256) tab[i] = GROUP_SET_EMPTY;
    if (threadIdx.x == 0) { s_count = 0; s_marker = 0; }
    if constexpr (FK == 2) {
        __shared__ int64_t set_lds[KEY_SET_MAX];
        kt.setup_in(fa.a, fa.b, q, set_lds);        // (its barrier covers the table too)
    } else {
        if constexpr (FK == 1) group_filter_bounds(fa, q, kt);
        __syncthreads();
    }
    volatile uint32_t *count = &s_count;

    const uint32_t P = a.P;
    uint32_t used = P;
    const uint32_t n_ranks = kt.empty() ? 0u : P;       // (block-uniform)
    for (uint32_t j = 0; j < n_ranks; ++j) {
        const uint32_t c = uniform_word(a.probe + (uint64_t)q * P + j);
        const uint64_t lbeg = uniform_word(a.list_off + c);
        const uint64_t len = uniform_word(a.list_off + c + 1) - lbeg;
        for (uint64_t w0 = (uint64_t)wave * 64; w0 < len; w0 += 256) {
            if (*count >= a.k) break;
            const uint64_t p = lbeg + w0;
            const uint64_t clip = len - w0 < 64 ? (1ull << (len - w0)) - 1ull : ~0ull;
            uint64_t win = group_images_window(a.valid_pos, a.bits, p, clip);
            if constexpr (FK != 0) {
                if (win) win &= kt.window(fa.key_pos, fa.elem_size == 4, fa.valid_pos, p, lane);
            }
            if (win == 0) continue;
            bool added = false;
            if ((win >> lane) & 1ull) added = group_set_insert(tab, &s_marker, (uint64_t)load_key_pos(a.key_pos, GW == 1, p + (uint64_t)lane));
            const uint32_t n_added = (uint32_t)__popcll(__ballot(added));
            if (n_added && lane == 0) atomicAdd(&s_count, n_added);
        }
        __syncthreads();
        const bool reached = *count >= a.k;
        __syncthreads();        // (nobody adds for rank j + 1 before everybody has read the count of rank j)
        if (reached) { used = j + 1 > a.p0 ? j + 1 : a.p0; break; }
    }
    if (threadIdx.x == 0) {
        a.nprobe_used[q] = used;
        const uint64_t at = (uint64_t)q * P + (used - 1);
        const uint32_t c = a.probe[at];
        a.n_cand[q] = a.cand_base[at] + (a.list_off[c + 1] - a.list_off[c]);
    }
}

template <int GW>
static hipError_t launch_group_expand_w(const GroupExpandArgs &a, const GroupFilterArgs *fa, hipStream_t s) {
    const dim3 grid(a.nq), block(256);
    const GroupFilterArgs none{};
    if (!fa) hipLaunchKernelGGL((group_expand_kernel<0, GW>), grid, block, 0, s, a, none);
    else if (fa->kind == 2) hipLaunchKernelGGL((group_expand_kernel<2, GW>), grid, block, 0, s, a, *fa);
    else hipLaunchKernelGGL((group_expand_kernel<1, GW>), grid, block, 0, s, a, *fa);
    return hipGetLastError();
}

hipError_t launch_group_expand(const GroupExpandArgs &a, const GroupFilterArgs *fa, hipStream_t s) {
    if (!a.probe || !a.cand_base || !a.list_off || !a.key_pos || !a.nprobe_used || !a.n_cand) return hipErrorInvalidValue;
    if (fa) {
        if (!fa->key_pos || !fa->a || fa->kind > 2 || (fa->kind != 0 && !fa->b)) return hipErrorInvalidValue;
        if (fa->elem_size != 4 && fa->elem_size != 8) return hipErrorInvalidValue;
    }
    if (a.nq == 0) return hipSuccess;
    if (a.P == 0 || a.p0 == 0 || a.p0 > a.P || a.k == 0 || a.k > 1024) return hipErrorInvalidValue;
    if (a.elem_size == 4) return launch_group_expand_w<1>(a, fa, s);
    if (a.elem_size == 8) return launch_group_expand_w<2>(a, fa, s);
    return hipErrorInvalidValue;
}

}  // namespace pqv
