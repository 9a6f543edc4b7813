// kernels_half_screen.hip -- the screened top-k route over a corpus of IEEE binary16 rows (pqv.h: half-precision corpora,
// rerank_mode 2).  The answer is stream_h_kernel's by definition -- the same keys, so the same merge -- and the screen
// only decides which rows the exact chain (chain_tile_h) is spent on.  The stored rows ARE the matrix operand: no image, no copy.
//
//   half_xs_kernel        once per searcher: xs[row] >= |x| (one f32 per storage row; +inf where the row holds Inf / NaN)
//   half_query_kernel     per call: q16 = f16(q 2^e), |q|^2, qs >= |q|; flags non-finite / zero / out-of-range queries "exact"
//   half_seed_kernel      tau_q = the k-th smallest exact distance among the first ~sqrt(candidates k) capped candidates in probe order (an
//                         upper bound of the final k-th distance); fewer than k candidates: "exact".  Counts the pairs per list.
//   half_scan_kernel      pair and work-item offsets per list;  half_scatter_kernel: the pairs bucketed by list
//   screen_h_kernel       item = (list, tile of <= 64 of its queries, segment of its rows): v_mfma_f32_32x32x16_f16, rows on the
//                         lane-owned side straight from global memory in operand layout, query images in LDS; survivors appended
//   survivor_h_kernel     per query: 64 survivors per wave and tile through chain_tile_h into WaveTopk; an "exact" query (or one
//                         whose survivor list overflowed) walks its probed lists as stream_h_kernel does
//
// Under a row mask (pqv_topk_masked_f16 / pqv_topk_masked_device_f16) the answer is masked_stream_h_kernel's and the
// same launches run with three differences: half_seed_masked_kernel takes tau from ALLOWED rows only, screen_h_kernel<.., true>
// tests the lane's own row against the mask image and skips a tile no bit of which is set, and survivor_h_kernel<.., true> walks
// an "exact" query's lists under the mask.
#include "half_tile.hpp"

namespace pqv {

constexpr uint32_t HS_SEG_ROWS = 1024;      // rows of one work item: 4 waves x 8 tiles of 32 rows

// the bound's constants for rows of `dim` values, dim_p = dim rounded up to 64
struct HalfBound { float eA, eB, eN, cm; };
__device__ __forceinline__ HalfBound half_bound(uint32_t dim) {
    const float u = 5.9604645e-8f, sd = sqrtf((float)dim) * 1.000001f;      // 2^-24
    const uint32_t dim_p = (dim + 63u) / 64u * 64u;
    HalfBound b;
    b.eA = 1.01f * 4.8828125e-4f + 4.76837158e-7f * sd + (float)(2u * dim_p + 16u) * u;      // 2^-11 image, 2^-21 sqrt(dim) subnormal image, accumulation
    b.eB = 6.1035156e-5f * sd * 1.001f;                                                        // 2^-14 sqrt(dim): subnormal row elements, should the pipe flush them
    b.eN = (float)(6u * dim + 128u) * 1.1920929e-7f;                                           // the norms' margins and the roundings of mid
    b.cm = (float)(dim / 4u + 16u) * 1.1920929e-7f;                                            // the reference chain (5.7)
    return b;
}
// summation margin of an f32 sum of `dim` squares, any order
__device__ __forceinline__ float half_norm_up(uint32_t dim) { return 1.0f + (float)(dim + 16u) * 1.1920929e-7f; }

// ------------------------------------------------------------------------------------
// xs[r] = sqrt(sum x^2) raised by its summation margin: one wave per row, 16-byte loads (dim % 8 == 0).  The square of a half is
// exact in f32 and never underflows; a non-finite sum <=> a non-finite element -> +inf, and the row always survives the screen.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_xs_kernel(const uint16_t *__restrict__ rows, uint64_t n, uint32_t dim, float *__restrict__ xs) {
    const int lane = threadIdx.x & 63;
    const uint64_t r = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= n) return;
    const uint16_t *x = rows + r * dim;
    float s = 0.0f;
    for (uint32_t c = lane; c < dim / 8; c += 64) {
        const Half8 v = load_h8<16>(x + c * 8, true);
        const float4 a = widen_lo4(v), b = widen_hi4(v);
        s += a.x * a.x; s += a.y * a.y; s += a.z * a.z; s += a.w * a.w;
        s += b.x * b.x; s += b.y * b.y; s += b.z * b.z; s += b.w * b.w;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    if (lane == 0) xs[r] = s <= 3.0e38f ? sqrtf(s) * half_norm_up(dim) : INFINITY;
}
hipError_t launch_half_xs(const uint16_t *rows, uint64_t n, uint32_t dim, float *xs, hipStream_t s) {
    if (n == 0) return hipSuccess;
    if (dim == 0 || dim % 8 != 0 || (n + 3) / 4 > 0x7FFFFFFFull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(half_xs_kernel, dim3((uint32_t)((n + 3) / 4)), dim3(256), 0, s, rows, n, dim, xs);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------
// half_query_kernel: one wave per query.  e_q maps the largest |q_i| into [2^7, 2^8) (the probe screen's scale); the image row is
// dim_p halves, zero behind dim.  qinfo = {|q|^2 as summed, 2^-e_q, qs >= |q|, tau (half_seed_kernel)}.  Also zeroes the call's
// counters: the survivor counts and the pair histogram.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_query_kernel(const HalfScreenArgs a) {
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < 2 * a.n_clusters; i += gridDim.x * 256) a.hist[i] = 0u;      // hist, cursor
    const int lane = threadIdx.x & 63;
    const uint32_t q = blockIdx.x * 4 + (threadIdx.x >> 6), dim = a.st.dim, dim_p = (dim + 63u) / 64u * 64u;
    if (q >= a.st.nq) return;
    const float *qv = a.st.queries + (uint64_t)q * dim;
    float m = 0.0f, s = 0.0f;
    bool bad = false;
    for (uint32_t e = lane; e < dim; e += 64) {
        const float v = qv[e];
        bad |= !(fabsf(v) <= 3.0e38f);
        m = fmaxf(m, fabsf(v));
        s += v * v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) { m = fmaxf(m, __shfl_xor(m, off, 64)); s += __shfl_xor(s, off, 64); }
    int ex = 0;
    (void)frexpf(m, &ex);                   // m = f 2^ex, f in [0.5, 1): m 2^(8 - ex) in [2^7, 2^8)
    const int e = 8 - ex;
    const bool exact = __ballot(bad) != 0ull || !(m > 0.0f) || !(s <= 3.0e38f) || e < -90 || e > 90;
    const float scale = exact ? 0.0f : ldexpf(1.0f, e);
    uint16_t *img = a.q16 + (uint64_t)q * dim_p;
    for (uint32_t i = lane; i < dim_p; i += 64) {
        const _Float16 h = (i < dim && !exact) ? (_Float16)(qv[i] * scale) : (_Float16)0.0f;
        img[i] = __builtin_bit_cast(uint16_t, h);
    }
    if (lane == 0) {
        a.qinfo[q] = make_float4(s, exact ? 0.0f : ldexpf(1.0f, -e), sqrtf(s) * half_norm_up(dim), INFINITY);
        a.qflag[q] = exact ? 1u : 0u;
        a.surv_cnt[q] = 0u;
    }
}

// ------------------------------------------------------------------------------------
// half_seed_kernel: one wave per query, 4 per block.  Candidate position p of a query lies in the probed list of the last rank
// whose first position is <= p (halving search over cand_base), so the seed rows are taken in PROBE ORDER across lists: a nearest
// list that is empty or holds one row changes nothing.  The k-th smallest key's distance is tau.
// ------------------------------------------------------------------------------------
template <int CGH, int S>
__global__ __launch_bounds__(256) void half_seed_kernel(const HalfScreenArgs a) {
    __shared__ float lds_all[4 * tile_words_h<CGH, false>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words_h<CGH, false>();
    const uint32_t q = blockIdx.x * 4 + wave, np = a.st.nprobe, k = a.st.k;
    if (q >= a.st.nq) return;
    const uint32_t *probe = a.st.probe + (uint64_t)q * np;
    const uint64_t *cbase = a.st.cand_base + (uint64_t)q * np;
    const uint32_t c_last = probe[np - 1];
    uint64_t total = cbase[np - 1] + (a.st.list_off[c_last + 1] - a.st.list_off[c_last]);
    if (total > a.st.max_pos) total = a.st.max_pos;
    bool exact = a.qflag[q] != 0u || total < (uint64_t)k;
    if (!exact) {
        // seeds + expected survivors ~ S + total k / S is smallest at S = sqrt(total k): whole tiles, at least max(k, 64), at most 2048
        const uint32_t least = k > 64u ? k : 64u;
        const uint32_t ideal = ((uint32_t)fminf(sqrtf((float)total * (float)k), 2048.0f) + 63u) & ~63u;
        const uint32_t want = ideal > least ? ideal : least;
        const uint32_t n_seed = total < (uint64_t)want ? (uint32_t)total : want;
        const float *qv = a.st.queries + (uint64_t)q * a.st.dim;
        WaveTopk<S> tk;
        tk.init();
        for (uint32_t t0 = 0; t0 < n_seed; t0 += 64) {
            const uint32_t nvalid = n_seed - t0 < 64u ? n_seed - t0 : 64u;
            const uint64_t p = t0 + ((uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1);
            uint32_t lo = 0, hi = np;
            while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (cbase[mid] <= p) lo = mid; else hi = mid; }
            const uint32_t my_srow = storage_row(a.st, a.st.list_off[probe[lo]] + (p - cbase[lo]));
            const float sum = chain_tile_h<CGH, false, 16>(a.st, lds, qv, my_srow, nvalid, lane);
            tk.offer((uint32_t)lane < nvalid ? l2_key(sum, p) : KEY_EMPTY, my_srow, k, lane);
        }
        const uint64_t kk = tk.kth(k);
        if (kk == KEY_EMPTY) exact = true;
        else if (lane == 0) a.qinfo[q].w = __uint_as_float((uint32_t)(kk >> 32));
    }
    if (exact) { if (lane == 0) a.qflag[q] = 1u; return; }        // (walked exactly: none of its pairs is screened)
    for (uint32_t j = lane; j < np; j += 64) atomicAdd(&a.hist[probe[j]], 1u);
}

// ------------------------------------------------------------------------------------
// half_seed_masked_kernel: half_seed_kernel under a row mask -- one wave per query, 4 per block.  The seed rows are the first
// n_seed ALLOWED candidates in probe order: the wave walks its probed lists rank by rank in 64-position windows of the mask image
// (two words, funnel-shifted: a list does not begin at a multiple of 64), drops the bits at or beyond the candidate cap, and
// compacts the set positions -- rank from mbcnt, through the first 256 words of the idle chain tile -- into a queue whose entries
// carry the LIST position (-> storage row) and the CANDIDATE position (-> key).  Whenever 64 are queued one chain tile runs; the
// walk stops at n_seed evaluated rows, or at the end of the capped walk, where what is left in the queue is the last tile.
// n_seed is half_seed_kernel's with the allowed candidates ESTIMATED as total x allowed_frac (the mask's allowed count over the
// searcher's positions: no second pass over the words); an estimate that is off costs survivors, never correctness.
//
// tau, the k-th smallest seed key's distance, is the distance of an allowed candidate below the cap with at least k - 1 allowed
// candidates at or below it: an UPPER BOUND OF THE MASKED k-th DISTANCE.  That is the property a threshold from sampled rows
// lacks on f32 (kernels_mask.hip: "a threshold from a row the mask excludes is no bound on the masked answer") and what lets the
// screen run under a mask here.  Fewer than k allowed candidates in the whole capped walk: the query is "exact" -- the survivor
// kernel walks it under the mask and finds n_found < k.
// Also adds the probe merge's uncapped total n_cand[q] to candidate_rows (a masked call's merge counts nothing itself).
// ------------------------------------------------------------------------------------
template <int CGH, int S>
__global__ __launch_bounds__(256) void half_seed_masked_kernel(const HalfScreenArgs a) {
    static_assert(tile_words_h<CGH, false>() >= WindowQueue<true>::SCRATCH, "the compaction needs 256 words of the tile area");
    __shared__ float lds_all[4 * tile_words_h<CGH, false>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words_h<CGH, false>();
    const uint32_t q = blockIdx.x * 4 + wave, np = a.st.nprobe, k = a.st.k;
    if (q >= a.st.nq) return;
    const uint32_t *probe = a.st.probe + (uint64_t)q * np;
    const uint64_t *cbase = a.st.cand_base + (uint64_t)q * np;
    unsigned long long *st = stats_slot(a.stats, q);
    if (st && a.n_cand && lane == 0) atomicAdd(&st[2], (unsigned long long)a.n_cand[q]);
    const uint32_t c_last = probe[np - 1];
    uint64_t total = cbase[np - 1] + (a.st.list_off[c_last + 1] - a.st.list_off[c_last]);
    if (total > a.st.max_pos) total = a.st.max_pos;
    bool exact = a.qflag[q] != 0u || total < (uint64_t)k;
    if (!exact) {
        const uint32_t least = k > 64u ? k : 64u;
        const uint32_t ideal = ((uint32_t)fminf(sqrtf((float)total * a.allowed_frac * (float)k), 2048.0f) + 63u) & ~63u;
        const uint32_t n_seed = ideal > least ? ideal : least;
        const float *qv = a.st.queries + (uint64_t)q * a.st.dim;
        WaveTopk<S> tk;
        tk.init();
        WindowQueue<true> wq;
        wq.cq = reinterpret_cast<uint32_t *>(lds);
        uint32_t n_have = 0;
        auto seed_tile = [&](const QueueTile &t) {      // entry: list position (below the searcher's positions), payload: candidate position
            const uint32_t my_srow = storage_row(a.st, t.my_r);
            const float sum = chain_tile_h<CGH, false, 16>(a.st, lds, qv, my_srow, t.nvalid, lane);
            tk.offer((uint32_t)lane < t.nvalid ? l2_key(sum, t.my_x) : KEY_EMPTY, my_srow, k, lane);
            n_have += t.nvalid;
        };
        for (uint32_t j = 0; j < np && n_have < n_seed; ++j) {
            const uint32_t c = probe[j];
            const uint64_t lbeg = a.st.list_off[c], cb = cbase[j];
            uint64_t len = a.st.list_off[c + 1] - lbeg;
            const uint64_t room = a.st.max_pos > cb ? a.st.max_pos - cb : 0;
            if (len > room) len = room;
            for (uint64_t w0 = 0; w0 < len && n_have < n_seed; w0 += 64) {
                const uint64_t clip = len - w0 < 64 ? (1ull << (len - w0)) - 1ull : ~0ull;
                const uint64_t win = image_window(a.mask_bits, lbeg + w0) & clip;
                const QueueTile t = wq.push(win, lbeg + w0, (uint32_t)(cb + w0) + (uint32_t)lane, lane);
                if (t.nvalid) seed_tile(t);
            }
        }
        if (n_have < n_seed) {          // the capped walk ended first: its last, partial tile
            const QueueTile t = wq.flush(lane);
            if (t.nvalid) seed_tile(t);
        }
        const uint64_t kk = tk.kth(k);
        if (kk == KEY_EMPTY) exact = true;
        else if (lane == 0) a.qinfo[q].w = __uint_as_float((uint32_t)(kk >> 32));
    }
    if (exact) { if (lane == 0) a.qflag[q] = 1u; return; }        // (walked exactly under the mask: none of its pairs is screened)
    for (uint32_t j = lane; j < np; j += 64) atomicAdd(&a.hist[probe[j]], 1u);
}

// ------------------------------------------------------------------------------------
// half_scan_kernel (one block): pair_off = exclusive sums of the histogram; item_off = exclusive sums of the lists' work items,
// ceil(pairs / qt) query tiles x ceil(rows / HS_SEG_ROWS) segments.  Thread t owns a contiguous run of lists.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void half_scan_kernel(const HalfScreenArgs a) {
    __shared__ uint32_t sp[256], si[256];
    const uint32_t kc = a.n_clusters, per = (kc + 255u) / 256u, t = threadIdx.x;
    const uint32_t c0 = t * per < kc ? t * per : kc, c1 = c0 + per < kc ? c0 + per : kc;
    auto items = [&](uint32_t c, uint32_t cnt) {
        const uint64_t len = a.st.list_off[c + 1] - a.st.list_off[c];
        return cnt ? (cnt + a.qt - 1u) / a.qt * (uint32_t)((len + HS_SEG_ROWS - 1u) / HS_SEG_ROWS) : 0u;
    };
    uint32_t np_ = 0, ni = 0;
    for (uint32_t c = c0; c < c1; ++c) { const uint32_t cnt = a.hist[c]; np_ += cnt; ni += items(c, cnt); }
    sp[t] = np_; si[t] = ni;
    __syncthreads();
    uint32_t bp = 0, bi = 0;
    for (uint32_t i = 0; i < t; ++i) { bp += sp[i]; bi += si[i]; }
    for (uint32_t c = c0; c < c1; ++c) {
        const uint32_t cnt = a.hist[c];
        a.pair_off[c] = bp; a.item_off[c] = bi;
        bp += cnt; bi += items(c, cnt);
    }
    if (t == 255) { a.pair_off[kc] = bp; a.item_off[kc] = bi; }       // (c1 == kc for the last thread: bp / bi are the totals)
}
__global__ __launch_bounds__(256) void half_scatter_kernel(const HalfScreenArgs a) {
    const uint32_t n_pairs = a.st.nq * a.st.nprobe;      // (hist[kc .. 2 kc): the lists' cursors)
    for (uint32_t p = blockIdx.x * 256 + threadIdx.x; p < n_pairs; p += gridDim.x * 256) {
        if (a.qflag[p / a.st.nprobe]) continue;
        const uint32_t c = a.st.probe[p];
        a.pairs[a.pair_off[c] + atomicAdd(&a.hist[a.n_clusters + c], 1u)] = p;
    }
}

// ------------------------------------------------------------------------------------
// screen_h_kernel<NQT>: a block takes work items (list c, query tile, row segment) in a grid-stride loop.
//   query side   the tile's images (up to 32 NQT queries) in LDS, rows of dim_p / 8 + 1 sixteen-byte units: the odd stride spreads
//                the 32 queries a read instruction touches over all banks.
//   row side     a wave owns 32 rows at a time; lane (r, h) reads 64 contiguous bytes of row r per 128-byte K stage -- the halves
//                h 32 + 8 c .. + 7 of the stage for c = 0 .. 3 -- straight into the B operand of step c, the next stage's loads
//                issued before this stage's matrix instructions.  K is a sum: both sides only have to agree on the order.  A
//                chunk at or beyond the row's own end is zero and is never loaded, so nothing is read behind a row's last byte.
//   epilogue     C / D column = lane & 31 is a DATA ROW: xs, the position and the decision are lane-local; register i of tile t is
//                query 32 t + (i & 3) + 8 (i >> 2) + 4 h.  mid = |q|^2 + xs^2 - 2 acc 2^-e, E = (|q|^2 + xs^2) eN + 2 qs (xs eA + eB),
//                lb = (mid - E) (1 - cm) where positive; a pair survives unless lb > tau (NaN survives; xs = +inf survives).
//   append       per register and half-wave one atomicAdd on the query's count, ranks from the ballot.
//   MASKED       the 32 mask bits of a wave's tile -- list positions lbeg + row0 .. + 31: two words of the image, funnel-shifted,
//                wave-uniform -- are loaded BEFORE the K loop and are in flight under it.  No bit set: the tile's loads, matrix
//                instructions and epilogue are skipped (a wave-uniform branch; no barrier lies inside the row loop).  Else the
//                epilogue's lane-local test gains one term, the lane's own bit: an excluded row survives for no query.
//                screened_pairs counts allowed rows only; the allowed pairs below the cap are the call's considered rows and go
//                to embeddings_fetched (a masked call's probe merge counts nothing).
// ------------------------------------------------------------------------------------
template <int NQT, bool MASKED = false>
__global__ __launch_bounds__(256) void screen_h_kernel(const HalfScreenArgs a) {
    constexpr int QT = 32 * NQT;
    extern __shared__ uint4 hs_q[];
    __shared__ float4 s_info[QT];
    __shared__ uint64_t s_cbase[QT];
    __shared__ uint32_t s_q[QT];
    __shared__ uint32_t s_item[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    const uint32_t dim = a.st.dim, nst = (dim + 63u) / 64u, qstride = nst * 8u + 1u, kc = a.n_clusters, np = a.st.nprobe;
    const HalfBound hb = half_bound(dim);
    const uint32_t n_items = a.item_off[kc];
    unsigned long long n_screened = 0;
    uint32_t n_considered = 0;              // MASKED: this lane's allowed pairs below the cap (< 2^32: a lane meets 16 NQT pairs per tile)

    for (uint32_t item = blockIdx.x; item < n_items; item += gridDim.x) {
        __syncthreads();                    // the previous item's LDS is read no more
        if (tid == 0) {
            uint32_t lo = 0, hi = kc - 1;   // the first list whose items end behind `item`
            while (lo < hi) { const uint32_t mid = (lo + hi) >> 1; if (a.item_off[mid + 1] > item) hi = mid; else lo = mid + 1; }
            s_item[0] = lo; s_item[1] = item - a.item_off[lo];
        }
        __syncthreads();
        const uint32_t c = s_item[0];
        const uint64_t lbeg = a.st.list_off[c], len = a.st.list_off[c + 1] - lbeg;
        const uint32_t nseg = (uint32_t)((len + HS_SEG_ROWS - 1u) / HS_SEG_ROWS);
        const uint32_t qtile = s_item[1] / nseg, seg = s_item[1] % nseg;
        const uint32_t p0 = a.pair_off[c] + qtile * QT, cnt = a.pair_off[c + 1] - p0;
        const uint32_t nqv = cnt < (uint32_t)QT ? cnt : (uint32_t)QT;
        if (tid < QT) {
            if ((uint32_t)tid < nqv) {
                const uint32_t pair = a.pairs[p0 + tid], q = pair / np;
                s_q[tid] = q; s_info[tid] = a.qinfo[q]; s_cbase[tid] = a.st.cand_base[pair];
            } else {
                s_q[tid] = 0xFFFFFFFFu;
            }
        }
        __syncthreads();
        for (uint32_t i = tid; i < (uint32_t)QT * nst * 8u; i += 256) {
            const uint32_t qs = i / (nst * 8u), ch = i - qs * (nst * 8u), q = s_q[qs];
            hs_q[qs * qstride + ch] = q != 0xFFFFFFFFu ? reinterpret_cast<const uint4 *>(a.q16 + (uint64_t)q * nst * 64u)[ch] : make_uint4(0u, 0u, 0u, 0u);
        }
        __syncthreads();

        const uint64_t s0 = (uint64_t)seg * HS_SEG_ROWS, s1 = s0 + HS_SEG_ROWS < len ? s0 + HS_SEG_ROWS : len;
        for (uint64_t row0 = s0 + (uint64_t)wave * 32; row0 < s1; row0 += 128) {
            const uint64_t lrow = row0 + (uint32_t)r;
            bool rvalid = lrow < s1;
            if constexpr (MASKED) {
                const uint32_t tile_bits = (uint32_t)image_window(a.mask_bits, lbeg + row0);       // (row0 < s1 <= len: a position of the image)
                if (__builtin_amdgcn_readfirstlane(tile_bits) == 0u) continue;
                rvalid = rvalid && ((tile_bits >> r) & 1u);
            }
            const uint32_t srow = storage_row(a.st, lbeg + (rvalid ? lrow : s1 - 1));
            const float xs = a.xs[srow];
            const uint16_t *xrow = a.st.mat_h + (uint64_t)srow * dim + (uint32_t)h * 32u;
            auto fetch = [&](uint32_t st, uint4 (&v)[4]) {
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const uint32_t k0 = st * 64u + (uint32_t)h * 32u + (uint32_t)cc * 8u;
                    v[cc] = k0 < dim ? *reinterpret_cast<const uint4 *>(xrow + st * 64u + cc * 8) : make_uint4(0u, 0u, 0u, 0u);
                }
            };
            f32x16_t acc[NQT];
#pragma unroll
            for (int t = 0; t < NQT; ++t)
#pragma unroll
                for (int i = 0; i < 16; ++i) acc[t][i] = 0.0f;
            const bool two = NQT > 1 && nqv > 32u;      // (block-uniform: the second query tile is empty otherwise)
            uint4 cur[4], nxt[4];
            fetch(0, cur);
            for (uint32_t st = 0; st < nst; ++st) {
                if (st + 1 < nst) fetch(st + 1, nxt);
                const uint4 *qrow = hs_q + (uint32_t)r * qstride + st * 8u + (uint32_t)h * 4u;
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) {
                    const f16x8_t bv = __builtin_bit_cast(f16x8_t, cur[cc]);
                    acc[0] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, qrow[cc]), bv, acc[0], 0, 0, 0);
                    if constexpr (NQT > 1) {
                        if (two) acc[1] = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, qrow[32u * qstride + cc]), bv, acc[1], 0, 0, 0);
                    }
                }
#pragma unroll
                for (int cc = 0; cc < 4; ++cc) cur[cc] = nxt[cc];
            }
            // ---- epilogue: the lane's row against the tile's queries
            const bool xinf = !(xs <= 3.0e38f);
            const float x2 = xs * xs, xe = xs * hb.eA + hb.eB;
            n_screened += (unsigned long long)__popcll(__ballot(rvalid && h == 0)) * nqv;
#pragma unroll
            for (int t = 0; t < NQT; ++t) {
                if (t == 1 && !two) break;
#pragma unroll
                for (int i = 0; i < 16; ++i) {
                    const uint32_t qs = (uint32_t)t * 32u + (uint32_t)((i & 3) + 8 * (i >> 2) + 4 * h);
                    bool keep = false;
                    uint64_t pos = 0;
                    if (qs < nqv && rvalid) {
                        const float4 qi = s_info[qs];       // {|q|^2, 2^-e, qs, tau}
                        pos = s_cbase[qs] + lrow;
                        const float n2 = qi.x + x2;
                        const float mid = n2 - 2.0f * (acc[t][i] * qi.y);
                        const float E = (n2 * hb.eN + 2.0f * qi.z * xe) * 1.00001f;
                        const float L = mid - E;
                        const float lb = L > 0.0f ? L * (1.0f - hb.cm) * 0.999999f : L;
                        keep = pos < a.st.max_pos && (xinf || !(lb > qi.w));
                        if constexpr (MASKED) n_considered += pos < a.st.max_pos ? 1u : 0u;
                    }
                    const uint64_t m = __ballot(keep);
                    if (m) {
                        const uint32_t mh = (uint32_t)(m >> (32 * h));
                        if (mh) {           // (the half-wave's lanes share the query)
                            const uint32_t q = s_q[qs];
                            const int leader = 32 * h + __builtin_ctz(mh);
                            uint32_t base = 0;
                            if (lane == leader) base = atomicAdd(&a.surv_cnt[q], (uint32_t)__popc(mh));
                            base = (uint32_t)__shfl((int)base, leader, 64);
                            const uint32_t at = base + (uint32_t)__popc(mh & ((1u << r) - 1u));
                            if (keep && at < a.surv_cap) a.surv[(uint64_t)q * a.surv_cap + at] = make_uint2((uint32_t)pos, srow);
                        }
                    }
                }
            }
        }
    }
    if (a.stats && lane == 0 && n_screened) atomicAdd(stats_slot(a.stats, blockIdx.x * 4 + wave), n_screened);
    if constexpr (MASKED) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) n_considered += (uint32_t)__shfl_xor((int)n_considered, off, 64);
        if (a.stats && lane == 0 && n_considered) atomicAdd(stats_slot(a.stats, blockIdx.x * 4 + wave) + 3, (unsigned long long)n_considered);
    }
}

// ------------------------------------------------------------------------------------
// survivor_h_kernel: grid (HS_PARTS / 4, nq); wave g of a query takes its survivors 64 at a time (tiles g, g + HS_PARTS, ...)
// through chain_tile_h, which gathers by storage row, and offers l2_key(sum, position): stream_h_kernel's keys.  A query flagged
// "exact", or whose count ran past the list, walks its probed lists instead (rank g, g + HS_PARTS, ...), positions below the cap.
// Every wave writes its list (empty ones too): the merge reads [nq][HS_PARTS][k].
// MASKED: the survivors are allowed rows already; the walk of an "exact" query is masked_stream_h_kernel's filtered walk over each
// of its lists (the window queue's compaction through the idle chain tile), so an excluded row is never loaded there either.  The
// rows such a walk evaluates are the considered rows of a query flagged "exact" -- none of its pairs was screened -- and go to
// embeddings_fetched; a query walked because its survivor list overflowed was counted by the screen.
// ------------------------------------------------------------------------------------
template <int CGH, int S, bool MASKED = false>
__global__ __launch_bounds__(256) void survivor_h_kernel(const HalfScreenArgs a) {
    static_assert(tile_words_h<CGH, false>() >= WindowQueue<false>::SCRATCH, "the compaction needs 128 words of the tile area");
    __shared__ float lds_all[4 * tile_words_h<CGH, false>()];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    float *lds = lds_all + wave * tile_words_h<CGH, false>();
    const uint32_t q = blockIdx.y, g = blockIdx.x * 4 + wave, np = a.st.nprobe, k = a.st.k;
    const float *qv = a.st.queries + (uint64_t)q * a.st.dim;
    const uint32_t cnt = a.surv_cnt[q];
    const bool exact = a.qflag[q] != 0u || cnt > a.surv_cap;
    WaveTopk<S> tk;
    tk.init();
    unsigned long long n_eval = 0;
    if (!exact) {
        const uint2 *sv = a.surv + (uint64_t)q * a.surv_cap;
        for (uint32_t t0 = g * 64u; t0 < cnt; t0 += HS_PARTS * 64u) {
            const uint32_t nvalid = cnt - t0 < 64u ? cnt - t0 : 64u;
            const uint2 e = sv[t0 + ((uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1)];
            const float sum = chain_tile_h<CGH, false, 16>(a.st, lds, qv, e.y, nvalid, lane);
            tk.offer((uint32_t)lane < nvalid ? l2_key(sum, e.x) : KEY_EMPTY, e.y, k, lane);
            n_eval += nvalid;
        }
    } else {
        for (uint32_t j = g; j < np; j += HS_PARTS) {
            const uint32_t c = a.st.probe[(uint64_t)q * np + j];
            const uint64_t lbeg = a.st.list_off[c], cb = a.st.cand_base[(uint64_t)q * np + j];
            uint64_t len = a.st.list_off[c + 1] - lbeg;
            const uint64_t room = a.st.max_pos > cb ? a.st.max_pos - cb : 0;
            if (len > room) len = room;
            if constexpr (MASKED) {
                n_eval += filtered_walk<false>(
                    lbeg, 0, len, lds, lane, [&](uint64_t p, uint64_t, uint64_t, uint32_t &) { return image_window(a.mask_bits, p); },
                    [&](const QueueTile &t) {
                        const uint32_t my_srow = storage_row(a.st, lbeg + t.my_r);
                        const float sum = chain_tile_h<CGH, false, 16>(a.st, lds, qv, my_srow, t.nvalid, lane);
                        tk.offer((uint32_t)lane < t.nvalid ? l2_key(sum, cb + t.my_r) : KEY_EMPTY, my_srow, k, lane);
                    });
            } else
            for (uint64_t t0 = 0; t0 < len; t0 += 64) {
                const uint32_t nvalid = len - t0 < 64 ? (uint32_t)(len - t0) : 64u;
                const uint32_t lrow = (uint32_t)lane < nvalid ? (uint32_t)lane : nvalid - 1;
                const uint32_t my_srow = storage_row(a.st, lbeg + t0 + lrow);
                const float sum = chain_tile_h<CGH, false, 16>(a.st, lds, qv, my_srow, nvalid, lane);
                tk.offer((uint32_t)lane < nvalid ? l2_key(sum, cb + t0 + (uint64_t)lane) : KEY_EMPTY, my_srow, k, lane);
                n_eval += nvalid;
            }
        }
    }
    write_partial_lists<S>(a.st.part_keys, a.st.part_vals, ((uint64_t)q * HS_PARTS + g) * k, k, lane, tk.key, tk.val);
    if (a.stats && lane == 0 && n_eval) atomicAdd(stats_slot(a.stats, q) + 1, n_eval);
    if constexpr (MASKED) {
        if (a.stats && lane == 0 && n_eval && a.qflag[q] != 0u) atomicAdd(stats_slot(a.stats, q) + 3, n_eval);
    }
}

// the whole route behind the probe: images, seeds, bucketing, screen, survivors (six launches on `s`); MASKED: under a.mask_bits
template <bool MASKED>
static hipError_t launch_half_screen_m(const HalfScreenArgs &a, hipStream_t s) {
    const StreamArgs &st = a.st;
    if (st.nq == 0) return hipSuccess;
    if (MASKED ? !a.mask_bits || !(a.allowed_frac >= 0.0f && a.allowed_frac <= 1.0f) : a.mask_bits != nullptr) return hipErrorInvalidValue;
    if (!st.mat_h || !st.probe || !st.cand_base || !st.list_off || !a.xs || st.dim == 0 || st.dim % 8 != 0 || st.k == 0 || st.k > 256 ||
        st.nprobe == 0 || st.nprobe > 1024 || a.n_clusters == 0 || (a.qt != 32 && a.qt != 64) || a.surv_cap == 0 || st.nq > 0xFFFFu ||
        (uint64_t)st.nq * st.nprobe > 0x7FFFFFFFull)
        return hipErrorInvalidValue;
    const uint32_t nst = (st.dim + 63) / 64;
    const size_t lds = (size_t)a.qt * (nst * 8 + 1) * 16;
    if (lds > half_screen_lds_max()) return hipErrorInvalidValue;
    const uint32_t qblocks = (st.nq + 3) / 4;
    hipLaunchKernelGGL(half_query_kernel, dim3(qblocks), dim3(256), 0, s, a);
    auto seed = [&](auto cgh, auto slots) {
        if constexpr (MASKED) hipLaunchKernelGGL((half_seed_masked_kernel<cgh.value, slots.value>), dim3(qblocks), dim3(256), 0, s, a);
        else hipLaunchKernelGGL((half_seed_kernel<cgh.value, slots.value>), dim3(qblocks), dim3(256), 0, s, a);
    };
    auto surv = [&](auto cgh, auto slots) { hipLaunchKernelGGL((survivor_h_kernel<cgh.value, slots.value, MASKED>), dim3(HS_PARTS / 4, st.nq), dim3(256), 0, s, a); };
    auto by_shape = [&](auto f) {
        using I = std::integral_constant<int, 1>; using IV = std::integral_constant<int, 4>;
        using C16 = std::integral_constant<int, 16>; using C32 = std::integral_constant<int, 32>;
        if (st.dim <= 128) { if (st.k <= 64) f(C16{}, I{}); else f(C16{}, IV{}); }
        else { if (st.k <= 64) f(C32{}, I{}); else f(C32{}, IV{}); }
    };
    by_shape(seed);
    hipLaunchKernelGGL(half_scan_kernel, dim3(1), dim3(256), 0, s, a);
    hipLaunchKernelGGL(half_scatter_kernel, dim3(std::min<uint32_t>(1024, (st.nq * st.nprobe + 255) / 256)), dim3(256), 0, s, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const void *kern = a.qt == 64 ? reinterpret_cast<const void *>(screen_h_kernel<2, MASKED>) : reinterpret_cast<const void *>(screen_h_kernel<1, MASKED>);
    e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) { (void)hipGetLastError(); return e; }
    if (a.qt == 64) hipLaunchKernelGGL((screen_h_kernel<2, MASKED>), dim3(1024), dim3(256), lds, s, a);
    else hipLaunchKernelGGL((screen_h_kernel<1, MASKED>), dim3(1024), dim3(256), lds, s, a);
    by_shape(surv);
    return hipGetLastError();
}
hipError_t launch_half_screen(const HalfScreenArgs &a, hipStream_t s) { return launch_half_screen_m<false>(a, s); }
// ... under a row mask: half_seed_masked_kernel, screen_h_kernel<.., true>, survivor_h_kernel<.., true>
hipError_t launch_half_screen_masked(const HalfScreenArgs &a, hipStream_t s) { return launch_half_screen_m<true>(a, s); }

}  // namespace pqv
