// wave_group_lists.hpp -- the wave-distributed lists of the distinct and grouped top-k, shared by the units that offer to them
// (kernels_distinct.hip, kernels_grouped.hip, kernels_distinct_filter.hip).  The invariants are stated in the first two.
#pragma once
#include "device_common.hpp"

namespace pqv {

// ------------------------------------------------------------------------------------
// Element e lives in slot e / 64, lane e % 64; ascending by key = (d2 bits << 32) | candidate position; grp[s][0 .. GW) are the
// 32-bit words of the entry's group value (GW = 1: an i32 column's value, GW = 2: the halves of an i64).  Entries at or beyond k
// are spill room, as in WaveTopk: they stay sorted and distinct but are never read out.
// ------------------------------------------------------------------------------------
template <int S, int GW>
struct WaveDistinctTopk {
    uint64_t key[S];
    uint32_t val[S];
    uint32_t grp[S][GW];

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int s = 0; s < S; ++s) {
            key[s] = KEY_EMPTY; val[s] = 0xFFFFFFFFu;
#pragma unroll
            for (int w = 0; w < GW; ++w) grp[s][w] = 0u;
        }
    }
    // key of element k-1 (the admission threshold); k is wave-uniform
    __device__ __forceinline__ uint64_t kth(uint32_t k) const {
        const uint32_t e = k - 1;
        uint64_t r = KEY_EMPTY;
#pragma unroll
        for (int s = 0; s < S; ++s)
            if ((int)(e >> 6) == s) r = readlane_u64(key[s], (int)(e & 63));
        return r;
    }
    // insert (x, xv, g), all wave-uniform, x < KEY_EMPTY
    __device__ __forceinline__ void insert(uint64_t x, uint32_t xv, const uint32_t (&g)[GW], int lane) {
        // the one filled slot of g's group, if any: a ballot per slot register, both halves of an i64 compared
        int e_old = -1;
        uint64_t old_key = KEY_EMPTY;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            bool same = key[s] != KEY_EMPTY;
#pragma unroll
            for (int w = 0; w < GW; ++w) same = same && grp[s][w] == g[w];
            const unsigned long long m = __ballot(same);
            if (m) {
                const int l = __builtin_ctzll(m);
                e_old = s * 64 + l;
                old_key = readlane_u64(key[s], l);
            }
        }
        if (e_old >= 0 && old_key < x) return;          // the group's entry is nearer: drop the candidate
        int p = 0;                                      // rank of x
#pragma unroll
        for (int s = 0; s < S; ++s) p += __popcll(__ballot(key[s] < x));
        // elements (p, hi] move up by one and x goes to p: hi = the group's old entry (p <= e_old: nothing falls off the end), or
        // the end of the list (WaveTopk::insert: the largest element is dropped)
        const int hi = e_old >= 0 ? e_old : S * 64 - 1;
#pragma unroll
        for (int s = S - 1; s >= 0; --s) {
            if (s * 64 > hi || s * 64 + 63 < p) continue;          // (wave-uniform) no element of this slot changes
            uint64_t up = shfl_up1_u64(key[s]);
            uint32_t upv = (uint32_t)__shfl_up((int)val[s], 1, 64);
            uint32_t upg[GW];
#pragma unroll
            for (int w = 0; w < GW; ++w) upg[w] = (uint32_t)__shfl_up((int)grp[s][w], 1, 64);
            if (s > 0) {
                const uint64_t pk = readlane_u64(key[s - 1], 63);
                const uint32_t pv = readlane_u32(val[s - 1], 63);
                uint32_t pg[GW];
#pragma unroll
                for (int w = 0; w < GW; ++w) pg[w] = readlane_u32(grp[s - 1][w], 63);
                if (lane == 0) {
                    up = pk; upv = pv;
#pragma unroll
                    for (int w = 0; w < GW; ++w) upg[w] = pg[w];
                }
            }
            const int e = s * 64 + lane;
            if (e > p && e <= hi) {
                key[s] = up; val[s] = upv;
#pragma unroll
                for (int w = 0; w < GW; ++w) grp[s][w] = upg[w];
            } else if (e == p) {
                key[s] = x; val[s] = xv;
#pragma unroll
                for (int w = 0; w < GW; ++w) grp[s][w] = g[w];
            }
        }
    }
    // offer one candidate per lane (mykey == KEY_EMPTY for lanes with none).  mykey < kth(k) stays the admission test: a candidate
    // at or above the k-th entry cannot improve a group that is in the first k, and cannot enter them otherwise.
    __device__ __forceinline__ void offer(uint64_t mykey, uint32_t myval, const uint32_t (&mygrp)[GW], uint32_t k, int lane) {
        uint64_t thr = kth(k);
        unsigned long long m = __ballot(mykey < thr);
        while (m) {
            const int L = __builtin_ctzll(m);
            const uint64_t x = readlane_u64(mykey, L);
            const uint32_t xv = readlane_u32(myval, L);
            uint32_t g[GW];
#pragma unroll
            for (int w = 0; w < GW; ++w) g[w] = readlane_u32(mygrp[w], L);
            insert(x, xv, g, lane);
            thr = kth(k);
            m &= m - 1;
            m &= __ballot(mykey < thr);
        }
    }
};

constexpr uint32_t GROUPED_SLOT_EMPTY = 0xFFFFFFFFu;

// ------------------------------------------------------------------------------------
// Element e lives in slot register e / 64, lane e % 64; ascending by (slot, key), key = (d2 bits << 32) | candidate position; the
// n filled elements are [0, n), everything behind them is (GROUPED_SLOT_EMPTY, KEY_EMPTY).  A group's entries are contiguous:
// group g's i-th nearest row is element (entries of slots < g) + i.
// ------------------------------------------------------------------------------------
template <int S>
struct WaveGroupedTopk {
    uint64_t key[S];
    uint32_t val[S];
    uint32_t slot[S];
    uint32_t n;         // filled elements (wave-uniform)

    __device__ __forceinline__ void init() {
#pragma unroll
        for (int s = 0; s < S; ++s) { key[s] = KEY_EMPTY; val[s] = 0xFFFFFFFFu; slot[s] = GROUPED_SLOT_EMPTY; }
        n = 0;
    }
    // insert (x, xv, sl), all wave-uniform, x < KEY_EMPTY, sl < k; m = group_size
    __device__ __forceinline__ void insert(uint64_t x, uint32_t xv, uint32_t sl, uint32_t m, int lane) {
        // slot sl's segment [lo, lo + cnt) and the rank of x inside it: three ballots per slot register
        int lo = 0, cnt = 0, below = 0;
#pragma unroll
        for (int s = 0; s < S; ++s) {
            lo += __popcll(__ballot(slot[s] < sl));
            cnt += __popcll(__ballot(slot[s] == sl));
            below += __popcll(__ballot(slot[s] == sl && key[s] < x));
        }
        const int p = lo + below;                       // rank of (sl, x)
        // elements (p, hi] move up by one and x goes to p.  The segment has room: hi = n, the first empty element (n < k * m <= S * 64
        // while some slot is short).  It is full: x replaces the segment's largest entry lo + cnt - 1, or is dropped when it is
        // not smaller than that (below == cnt).
        int hi;
        if ((uint32_t)cnt < m) {
            hi = (int)n;
            if (hi >= S * 64) return;                   // (never: only members are offered)
            ++n;
        } else {
            if (below == cnt) return;
            hi = lo + cnt - 1;
        }
#pragma unroll
        for (int s = S - 1; s >= 0; --s) {
            if (s * 64 > hi || s * 64 + 63 < p) continue;          // (wave-uniform) no element of this slot register changes
            uint64_t up = shfl_up1_u64(key[s]);
            uint32_t upv = (uint32_t)__shfl_up((int)val[s], 1, 64);
            uint32_t ups = (uint32_t)__shfl_up((int)slot[s], 1, 64);
            if (s > 0) {
                const uint64_t pk = readlane_u64(key[s - 1], 63);
                const uint32_t pv = readlane_u32(val[s - 1], 63);
                const uint32_t ps = readlane_u32(slot[s - 1], 63);
                if (lane == 0) { up = pk; upv = pv; ups = ps; }
            }
            const int e = s * 64 + lane;
            if (e > p && e <= hi) { key[s] = up; val[s] = upv; slot[s] = ups; }
            else if (e == p) { key[s] = x; val[s] = xv; slot[s] = sl; }
        }
    }
    // offer one candidate per lane (mykey == KEY_EMPTY for lanes with none)
    __device__ __forceinline__ void offer(uint64_t mykey, uint32_t myval, uint32_t myslot, uint32_t m, int lane) {
        unsigned long long todo = __ballot(mykey != KEY_EMPTY);
        while (todo) {
            const int L = __builtin_ctzll(todo);
            insert(readlane_u64(mykey, L), readlane_u32(myval, L), readlane_u32(myslot, L), m, lane);
            todo &= todo - 1;
        }
    }
};

}  // namespace pqv
