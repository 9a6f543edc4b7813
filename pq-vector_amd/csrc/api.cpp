// api.cpp -- the C ABI of include/pqv.h: host orchestration of the gfx950 kernels.
//
// Host logic mirrored here (reference paths):
//   build_ivf_index / k_means / sample_embeddings   src/ivf/index.rs:152-214,222-242,323-457
//   IvfIndex::{to_bytes,from_bytes,candidate_rows}    src/ivf/index.rs:57-128
//   topk()                                            src/ivf/search.rs:83-142
// There is no CPU compute fallback: distances, argmins and top-k selection only ever run
// in the HIP kernels of kernels_*.hip; the host draws the seeded choices, walks the two
// order-sensitive f32 scalar scans of k-means++ (index.rs:370-383) and moves bytes.
#include "../../include/pqv.h"

#include <hip/hip_runtime.h>
#include <time.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <functional>
#include <system_error>
#include <thread>
#include <cmath>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <type_traits>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "internal.h"
#include "kernels.h"
#include "rng.hpp"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string &msg) {
    g_last_error = msg;
    return code;
}

#define HIP_TRY(expr)                                                                     \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess) {                                                           \
            (void)hipGetLastError();   /* the runtime's sticky last-error must not leak into the next call */ \
            return fail(_e == hipErrorOutOfMemory ? PQV_ERR_OOM : PQV_ERR_HIP,            \
                        std::string(#expr) + ": " + hipGetErrorString(_e));              \
        }                                                                                 \
    } while (0)

// No C++ exception may cross the C ABI: every entry point runs its body through guard().
template <class F>
int guard(F &&body) noexcept {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        return fail(PQV_ERR_OOM, "host allocation failed");
    } catch (const std::exception &e) {
        return fail(PQV_ERR_INVALID, std::string("internal error: ") + e.what());
    } catch (...) {
        return fail(PQV_ERR_INVALID, "internal error");
    }
}

// A few streams per device made (and their hardware queues set up by an empty launch) at the library's first call for the device;
// a searcher takes its stream from here and gives it back -- made right after a build, a stream costs 10+ ms (the driver is still
// unmapping what the build freed).
struct StreamPool {
    std::mutex mu;
    std::vector<hipStream_t> idle[64];
};
static StreamPool &stream_pool() { static StreamPool *p = new StreamPool(); return *p; }     // (never destroyed: streams outlive static teardown order)
static hipError_t pool_get(int device, hipStream_t *out) {
    if (device >= 0 && device < 64) {
        StreamPool &sp = stream_pool();
        std::lock_guard<std::mutex> lock(sp.mu);
        if (!sp.idle[device].empty()) { *out = sp.idle[device].back(); sp.idle[device].pop_back(); return hipSuccess; }
    }
    return hipStreamCreateWithFlags(out, hipStreamNonBlocking);
}
static void pool_put(int device, hipStream_t s) {
    if (!s) return;
    if (device >= 0 && device < 64) {
        (void)hipStreamSynchronize(s);
        StreamPool &sp = stream_pool();
        std::lock_guard<std::mutex> lock(sp.mu);
        if (sp.idle[device].size() < 8) { sp.idle[device].push_back(s); return; }
    }
    (void)hipStreamDestroy(s);
}

int use_device(int device) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(PQV_ERR_NO_DEVICE,
                    "no HIP device available: libpqv_hip has no CPU fallback (gfx950 required)");
    if (device < 0 || device >= count)
        return fail(PQV_ERR_NO_DEVICE, "device index " + std::to_string(device) +
                                           " out of range (" + std::to_string(count) + " devices)");
    HIP_TRY(hipSetDevice(device));
    // The first call for a device loads the kernels' code objects (the runtime would otherwise do it inside whatever launches a unit's
    // first kernel: 7-8 ms of the first index build).  PQV_LAZY_INIT=1 leaves it to the runtime.
    static std::once_flag warmed[64];
    static const bool lazy = [] { const char *e = std::getenv("PQV_LAZY_INIT"); return e && *e == '1'; }();
    if (!lazy && device < 64)
        std::call_once(warmed[device], [] {
            (void)pqv::touch_probe(nullptr); (void)pqv::touch_screen(nullptr); (void)pqv::touch_brute(nullptr); (void)pqv::touch_build(nullptr);
            (void)pqv::touch_layout(nullptr); (void)pqv::touch_list(nullptr); (void)pqv::touch_kpp(nullptr); (void)pqv::touch_range(nullptr); (void)pqv::touch_mask(nullptr); (void)pqv::touch_predicate(nullptr);
            (void)pqv::touch_partition_range(nullptr);
            (void)hipStreamSynchronize(nullptr);
            // ... and the runtime's staging buffers for copies from / to pageable host memory are made by the first such copies
            void *d = nullptr;
            if (hipMalloc(&d, 1 << 20) == hipSuccess) {
                std::vector<char> h(1 << 20, 0);
                (void)hipMemcpy(d, h.data(), h.size(), hipMemcpyHostToDevice);
                (void)hipMemcpy(h.data(), d, h.size(), hipMemcpyDeviceToHost);
                (void)hipFree(d);
            }
            for (int i = 0; i < 2; ++i) {
                hipStream_t st = nullptr;
                if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) break;
                (void)pqv::touch_build(st);
                int dev = -1;
                (void)hipGetDevice(&dev);
                pool_put(dev, st);
            }
            (void)hipGetLastError();
        });
    return PQV_OK;
}

// RAII device buffer
bool verbose();
double now_s();
// PQV_VERBOSE: seconds and calls spent in hipMalloc / hipFree since the last report (the build prints them)
static thread_local double g_alloc_s = 0.0, g_free_s = 0.0;
static thread_local unsigned g_alloc_n = 0, g_free_n = 0;
struct DevBuf {
    void *p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (!p) return;
        const bool vb = verbose();
        const double t0 = vb ? now_s() : 0.0;
        (void)hipFree(p); p = nullptr; bytes = 0;
        if (vb) { g_free_s += now_s() - t0; ++g_free_n; }
    }
    hipError_t alloc(size_t n) {
        release();
        if (n == 0) n = 16;
        const bool vb = verbose();
        const double t0 = vb ? now_s() : 0.0;
        hipError_t e = hipMalloc(&p, n);
        if (vb) { g_alloc_s += now_s() - t0; ++g_alloc_n; }
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    // grow-only
    hipError_t ensure(size_t n) { return (n <= bytes && p) ? hipSuccess : alloc(n + n / 4); }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

struct PinnedBuf {
    void *p = nullptr;
    size_t bytes = 0;
    ~PinnedBuf() { if (p) (void)hipHostFree(p); }
    hipError_t ensure(size_t n) {
        if (n <= bytes && p) return hipSuccess;
        if (p) { (void)hipHostFree(p); p = nullptr; bytes = 0; }
        hipError_t e = hipHostMalloc(&p, n ? n : 16, hipHostMallocDefault);
        if (e == hipSuccess) bytes = n; else p = nullptr;
        return e;
    }
    template <class T> T *as() const { return static_cast<T *>(p); }
};

// phase wall times of this thread's last index build (pqv_index_build_stats; bench.py's build_record unpacks the slots by position)
// FORM: an AssignLadder::Tier -- the one that decided the final assignment, the one Lloyd chose.  WIDE: assign_wide_kernel in the
// final assignment -- seconds between HIP events, launches.
enum BuildStat { BS_KPP_S, BS_LLOYD_S, BS_ITERS, BS_FINAL_ASSIGN_S, BS_HOST_LISTS_S, BS_FINAL_FORM, BS_LLOYD_FORM, BS_SAMPLE_ROWS,
                 BS_WIDE_KERNEL_S, BS_WIDE_LAUNCHES, BS_COUNT };
thread_local double g_build_stats[BS_COUNT] = {};

// PQV_VERBOSE=1: phase timings of the build on stderr
bool verbose() {
    static const bool v = [] { const char *e = std::getenv("PQV_VERBOSE"); return e && *e && *e != '0'; }();
    return v;
}
double now_s() {
    timespec ts;
    clock_gettime(CLOCK_MONOTONIC, &ts);
    return ts.tv_sec + ts.tv_nsec * 1e-9;
}

uint32_t host_workers() {
    long n = sysconf(_SC_NPROCESSORS_ONLN);
    return n > 0 ? static_cast<uint32_t>(n) : 1u;
}

}  // namespace

namespace pqv_internal {
int fail(int code, const std::string &msg) { return ::fail(code, msg); }
int use_device(int device) { return ::use_device(device); }
}  // namespace pqv_internal

// ---------------------------------------------------------------------------------------
// handles
// ---------------------------------------------------------------------------------------
// the device copy of the inverted lists a build leaves behind (40 MB per 10 M rows, freed with the index): a searcher made on the
// same device takes its row ids from it instead of uploading them again
struct DevRows {
    void *p = nullptr;
    int device = -1;
    uint64_t n = 0;
    ~DevRows() { if (p) { int cur = -1; (void)hipGetDevice(&cur); if (hipSetDevice(device) == hipSuccess) (void)hipFree(p); if (cur >= 0) (void)hipSetDevice(cur); } }
};
// The index' lists as its callers see them: the host vector, plus -- after a build -- the device copy it has NOT been downloaded
// from yet.  A build leaves the lists where it sorted them (4 bytes per row of HBM, freed with the last owner); the host copy is
// made by the first call that reads it (the blob writer, pqv_index_list_rows, a searcher's host-side calls, a searcher on another
// device).  Shared by the index and its searchers.
struct ListRows {
    std::mutex mu;
    std::vector<uint32_t> host;
    std::shared_ptr<DevRows> dev;
    uint64_t n = 0;
    bool pending = false;             // host is still empty: dev holds the lists
    // the host vector, downloaded now if it has to be (nullptr + fail() if that goes wrong)
    const std::vector<uint32_t> *get() {
        std::lock_guard<std::mutex> lock(mu);
        if (pending) {
            int cur = -1;
            (void)hipGetDevice(&cur);
            hipError_t e = hipSetDevice(dev->device);
            if (e == hipSuccess) {
                try { host.resize(n); } catch (const std::bad_alloc &) { if (cur >= 0) (void)hipSetDevice(cur); (void)fail(PQV_ERR_OOM, "host allocation failed"); return nullptr; }
                e = hipMemcpy(host.data(), dev->p, n * sizeof(uint32_t), hipMemcpyDeviceToHost);
            }
            if (cur >= 0) (void)hipSetDevice(cur);
            if (e != hipSuccess) { host.clear(); (void)fail(PQV_ERR_HIP, std::string("download of the inverted lists: ") + hipGetErrorString(e)); return nullptr; }
            pending = false;
        }
        return &host;
    }
};
struct pqv_index {
    uint32_t dim = 0;
    uint32_t n_clusters = 0;
    std::vector<float> centroids;     // [n_clusters * dim]
    std::vector<uint64_t> list_off;   // [n_clusters + 1]
    // concatenated inverted lists (see ListRows); `list_rows` is the host vector for the code that FILLS it -- readers go through rows->get()
    std::shared_ptr<ListRows> rows{std::make_shared<ListRows>()};
    std::vector<uint32_t> &list_rows{rows->host};
    uint64_t n_rows() const { return rows->pending ? rows->n : rows->host.size(); }
    uint64_t permutation_of = 0;      // != 0: the lists are a permutation of [0, permutation_of) by construction (a build's result)
    // largest indexed row id + 1 (pqv_index_append: new rows start at or above it, so a list extended at its end stays ascending):
    // set by a build (n) and by an append (first_row + n_rows); an index made from parts or bytes finds it by one host scan on first need
    mutable std::mutex bound_mu;
    mutable uint64_t bound = 0;
    mutable bool bound_known = false;
    void set_row_bound(uint64_t b) { bound = b; bound_known = true; }
    bool row_bound(uint64_t *out) const {      // false + fail() if the lists could not be read
        std::lock_guard<std::mutex> lock(bound_mu);
        if (!bound_known) {
            const std::vector<uint32_t> *rv = rows->get();
            if (!rv) return false;
            uint64_t b = 0;
            for (uint32_t r : *rv) b = std::max<uint64_t>(b, static_cast<uint64_t>(r) + 1);
            bound = b; bound_known = true;
        }
        *out = bound;
        return true;
    }
    bool known_row_bound(uint64_t *out) const {      // the bound where it is known already (no read of the lists)
        std::lock_guard<std::mutex> lock(bound_mu);
        if (bound_known) *out = bound;
        return bound_known;
    }
    pqv_index() = default;
    pqv_index(const pqv_index &) = delete;
    pqv_index &operator=(const pqv_index &) = delete;
};

// pinned staging buffers of the streaming upload (pqv_corpus_write_rows): a buffer is free, being filled by a caller, or in
// flight behind its event
struct UploadStage {
    static constexpr int N = 16;                  // (a page-level reader hands over ~1 MB pages from eight threads: many small buffers)
    static constexpr size_t BYTES = 8u << 20;
    std::mutex mu;
    std::condition_variable cv;
    void *pin[N] = {};
    void *dev64[N] = {};                          // f64 batches: device-side landing area of the same size (made on first use)
    hipEvent_t ev[N] = {};
    int state[N] = {};                            // 0 free, 1 claimed, 2 in flight
    static constexpr int NS = 4;                  // copy streams, slot i uses stream i % NS: several DMA operations in flight (1 MB pages: the
                                                  // per-operation overhead of ONE engine capped the loader at ~15 GB/s)
    hipStream_t copy_stream[NS] = {};
    ~UploadStage() {
        for (int i = 0; i < N; ++i) {
            if (ev[i]) (void)hipEventDestroy(ev[i]);
            if (pin[i]) (void)hipHostFree(pin[i]);
            if (dev64[i]) (void)hipFree(dev64[i]);
        }
        for (int i = 0; i < NS; ++i) if (copy_stream[i]) (void)hipStreamDestroy(copy_stream[i]);
    }
};

struct pqv_corpus {
    int device = 0;
    uint32_t dim = 0;
    uint64_t n = 0;
    uint64_t capacity = 0;
    float *d_rows = nullptr;  // [capacity, dim]
    bool owned = true;
    hipStream_t stream = nullptr;
    std::unique_ptr<UploadStage> upload;       // made by the first pqv_corpus_write_rows
    std::mutex upload_mu;
    // lazily computed per-row auxiliaries of pqv_brute_topk: 1/|v| and |v|^2
    mutable std::mutex aux_mu;
    mutable DevBuf aux_rnorm, aux_norm2, aux_v16;      // aux_v16: L2-normalised f16 images [n, dim_p] (the f16 screen of pqv_brute_topk)
    mutable uint64_t aux_rnorm_rows = 0, aux_norm2_rows = 0, aux_v16_rows = 0;
    mutable DevBuf aux_v8_max;                         // [12, nine used] maxima over the rows (kernels.h: BruteF16Args::row_max)
    mutable DevBuf aux_v8, aux_v8_sr, aux_v8_n;        // int8 images [n, dim_p8] + {1 / S, residual, mid-range, sum} + norm per row (the int8 screen of pqv_brute_topk)
    mutable uint64_t aux_v8_rows = 0;
    ~pqv_corpus() {
        if (d_rows && owned) (void)hipFree(d_rows);
        if (stream) (void)hipStreamDestroy(stream);
    }
};

// Per-call device scratch of a searcher (see pqv_searcher::lanes).
constexpr int PQV_LANES = 4;
struct Scratch {
    DevBuf s_probe_keys, s_probe_vals, s_probe, s_cand_base, s_ncand, s_part_keys, s_part_vals, s_queries, s_rows,
        s_dist, s_nfound, s_pair_u32, s_pairs, s_groups, s_quads, s_items, s_ticket, s_ticket2, s_cand_keys, s_cand_vals, s_cand_cnt, s_spilled,
        s_seed_ub, s_qblk, s_gthr, s_tie, s_replay, s_qnorm, s_qmax, s_thr_hist, s_thr_bins, s_qi8, s_qn2i, s_qres, s_qresu, s_pair_lb, s_part_flags, s_qpad, s_cand_lb, s_pendv, s_work, s_nwork, s_out,
        s_hit_cnt, s_hit_keys, s_hit_vals, s_alt_keys, s_alt_vals, s_rsegs, s_rout_off, s_rout_rows, s_rout_dist,   // s_hit_* .. s_rout_*: pqv_range_search
        s_pair_end, s_file_cnt,     // round-robin capped tables: per-pair candidate ends, per-file counts (SegProbeArgs)
        s_qcos,                     // PQV_COSINE: the call's normalised queries n(q), read by the cosine searcher's kernels
        s_qkeys,                    // keyed host calls (pqv_row_keys): the sub-batch's query keys, i64 [b]
        s_qfilt_a, s_qfilt_b,       // filtered host calls (pqv_key_filter): the sub-batch's a / b -- RANGE: lo, hi i64 [b]; IN: lims rebased to the
                                    // sub-batch u64 [b + 1], its slice of the values
        s_part_grp, s_grp_out,      // distinct calls: the partial lists' group values i64 [nq][n_part][k]; the host form's group_key block
        // grouped calls (pqv_topk_grouped): pass 1's rows / distances [nq][k] (not reported), its group values and n_found where the caller
        // takes none, the sorted sets [nq][k], the partial lists' slots [nq][n_part][k * group_size] and lengths [nq][n_part], and the
        // host form's group_rows block
        s_g1_rows, s_g1_dist, s_g1_keys, s_g1_nfound, s_gset_keys, s_gset_slot, s_gpart_slot, s_gpart_cnt, s_grows_out,
        s_expand_cnt, s_expand_used,    // pqv_topk_expand: the passing rows per probed list u32 [nq][P]; nprobe_used u32 [nq] where the caller takes none
        s_depths, s_depth_d2, s_depth_end,  // pqv_topk_depth: a host call's given depths u32 [b]; the probe distances' bits u32 [nq][P]; the pairs' candidate ends u64 [nq][P]
        s_ps_q16, s_ps_qn2, s_ps_score, // screened probe: the batch's query images f16 [nq][dim_p], |q - mean|^2 [nq], the scores f32 [nq][kc_pad]
        s_seg_off,                      // pqv_range_search_partition: the group's packed segment offsets u64 [b]
        s_pt_beg, s_pt_end, s_pt_nspan, // pqv_topk_partition: the spans' first entries u32 [nq] (IN: [nq][1024]), IN: their prefix sums and counts
        s_mmr_rows, s_mmr_dist, s_mmr_nf;   // pqv_topk_mmr: stage 1's rows u32 / distances f32 [nq][fetch_k] and n_found u32 [nq]; pqv_mmr_select's host form: the candidates
    PinnedBuf h_io;                 // small host calls: queries in, one block of results out, through pinned memory
    hipEvent_t done = nullptr;      // recorded after the last kernel of the call that used this lane
    hipStream_t stream = nullptr;   // the stream of that call
    bool used = false;
    // the lane's side stream for the wide-quad launch of a batch (TileArgs::side_stream), created on first use
    hipStream_t side = nullptr;
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    // every DevBuf above, for pqv_searcher_footprint (a buffer added to the declaration belongs here too)
    std::vector<const DevBuf *> bufs() const {
        return {&s_probe_keys, &s_probe_vals, &s_probe, &s_cand_base, &s_ncand, &s_part_keys, &s_part_vals, &s_queries, &s_rows,
                &s_dist, &s_nfound, &s_pair_u32, &s_pairs, &s_groups, &s_quads, &s_items, &s_ticket, &s_ticket2, &s_cand_keys, &s_cand_vals, &s_cand_cnt, &s_spilled,
                &s_seed_ub, &s_qblk, &s_gthr, &s_tie, &s_replay, &s_qnorm, &s_qmax, &s_thr_hist, &s_thr_bins, &s_qi8, &s_qn2i, &s_qres, &s_qresu, &s_pair_lb, &s_part_flags, &s_qpad, &s_cand_lb, &s_pendv, &s_work, &s_nwork, &s_out,
                &s_hit_cnt, &s_hit_keys, &s_hit_vals, &s_alt_keys, &s_alt_vals, &s_rsegs, &s_rout_off, &s_rout_rows, &s_rout_dist,
                &s_pair_end, &s_file_cnt, &s_qcos, &s_qkeys, &s_qfilt_a, &s_qfilt_b, &s_part_grp, &s_grp_out,
                &s_g1_rows, &s_g1_dist, &s_g1_keys, &s_g1_nfound, &s_gset_keys, &s_gset_slot, &s_gpart_slot, &s_gpart_cnt, &s_grows_out,
                &s_expand_cnt, &s_expand_used, &s_depths, &s_depth_d2, &s_depth_end, &s_ps_q16, &s_ps_qn2, &s_ps_score, &s_seg_off, &s_pt_beg, &s_pt_end, &s_pt_nspan,
                &s_mmr_rows, &s_mmr_dist, &s_mmr_nf};
    }
    ~Scratch() {
        if (done) (void)hipEventDestroy(done);
        if (ev_fork) (void)hipEventDestroy(ev_fork);
        if (ev_join) (void)hipEventDestroy(ev_join);
        if (side) (void)hipStreamDestroy(side);
    }
};

struct pqv_searcher {
    int device = 0;
    uint64_t uid = 0;                      // unique per searcher made in this process (a pqv_row_mask remembers its searcher by it)
    uint32_t dim = 0, n_clusters = 0;
    // storage dimension of the IVF-ordered rows: dim, or dim zero-padded to a multiple of 64 / 128 / 256 where the MFMA
    // screen has no tiling for dim itself (dim % 4 == 0; kernels_layout.hip: pad_rows_kernel -- distances stay bit-identical).
    // Everything downstream of the probe (blocked copies, screen, exact evaluation, replays) works on sdim-wide rows
    // and sdim-wide copies of the batch's queries.
    uint32_t sdim = 0;
    uint64_t n = 0;
    uint64_t max_list_len = 0;
    pqv_corpus *corpus = nullptr;          // borrowed
    std::vector<uint64_t> h_list_off;      // host copy for candidate_rows
    std::shared_ptr<ListRows> h_rows;      // the index' lists (shared, not copied; the host copy is made by the first call that reads it)
    DevBuf d_cent_t;                   // [dim/4][kc_pad] float4 transpose of the centroids (probe_rows_kernel), dim % 4 == 0
    uint32_t kc_pad = 0;
    // the screened batched probe (probe_screen_kernel + probe_resolve_kernel): the centroid mean, f16 images of (centroid - mean) at
    // ONE table-wide scale padded to a multiple of 64 values, |centroid - mean|^2, and the bound's constants; ps.ok: the table is
    // finite and its scale representable
    DevBuf d_ps_mu, d_ps_c16, d_ps_cn2;
    mutable DevBuf d_ps_stats;             // PQV_PROBE_SCREEN_STATS=1 (diagnostic): {queries, exact evaluations, all-exact queries}, printed by destroy
    struct ProbeScreen { bool ok = false, tried = false; uint32_t dim_p = 0; float inv_cs = 0, fn = 0, e1 = 0, e2s = 0, kS = 0, lo_f = 0, hi_f = 0; } ps;
    DevBuf d_centroids, d_list_off, d_ids, d_mat_ivf, d_stats;
    mutable DevBuf d_row_norm2;            // |x|^2 per storage row (f32 / f16 MFMA screens; see norms_done)
    const float *d_mat = nullptr;          // row storage the re-rank reads
    const uint32_t *d_row_of = nullptr;    // list position -> storage row (ROW_ORDER layout, and the images-only IVF layout)
    const uint32_t *d_final_ids = nullptr; // storage row -> file row id (IVF layout with its own f32 copy)
    // IVF-ordered layout WITHOUT a second f32 copy of the corpus (round 4): everything the screen streams -- the blocked operand
    // images, row terms and norms -- is in list order, while the exact evaluations (0.03 % of the pairs, the seed refinement, tie
    // replays) read the caller's row-order matrix through d_row_of.  Footprint 2.28 x -> 1.28 x the corpus on C3, and searcher
    // creation no longer allocates and writes n x dim floats.
    bool images_only = false;
    hipStream_t stream = nullptr;
    // scratch (guarded by mu): PQV_LANES independent sets, one per stream in use, so calls enqueued on
    // different streams overlap on the GPU (the tail of one batch's screen kernel is filled by the next
    // batch's probe / bucketing / seed kernels) instead of serialising on shared buffers
    mutable std::mutex mu;
    mutable Scratch lanes[PQV_LANES];
    // {wide items, of which in single-quad lists} of a recent batch, written by pair_scan_kernel straight into this pinned
    // buffer (a hint for the NEXT batch's cache policy, read without synchronisation -- wide_rows_nt)
    mutable PinnedBuf h_wide_stats;
    mutable uint32_t lane_rr = 0;
    // blocked MFMA-operand copies of the lists, one per operand form in use (0 f32, 1 f16, 2 int8); built at creation
    // for the form the dispatch rule picks, a second form only if a later call asks for it (e.g. k > 32 on short lists)
    mutable DevBuf d_mat_blk_op[3], d_blk_off;
    // f16 operands for the wide screened path: values * f16_scale rounded to f16; possible when the stored rows
    // are finite and the power-of-two scale and its square are representable
    mutable bool f16_ok = false;
    mutable float f16_scale = 1.0f;
    // The rows' squared norms and their maximum (-> f16_ok / f16_scale) are one pass over the corpus that the int8 screen never
    // reads: where the int8 copy is built at creation they are left to the first call that needs them (ensure_row_norms).
    mutable bool norms_done = false;
    mutable std::mutex norms_mu;
    uint64_t n_storage = 0;
    // int8 operands (rows of a multiple of 256 dims): per LIST the images of (x - centre_c) * S_c -- the IVF residual:
    // centre_c the per-dimension mid-range of the list's rows, S_c mapping the list's largest |x - centre_c| component
    // to 127 -- per row |xi|^2 and an upper bound of the residual norm, per list a radius >= |x - centre_c| (see
    // kernels_layout.hip: block_rows_i8_kernel); built with the blocked copy (ensure_blocked_copy)
    mutable bool i8_ok = false;
    // i8_residual: the per-list (residual) form pays where the lists are much tighter than the corpus (clustered data:
    // a per-list scale twice the global one halves the bound's slack); where they are not (uniform data) the one-centre
    // form gives the same bound with ONE image per query instead of one per probed pair -- 0.45 GB less traffic per
    // C3 step and an L2-hot staging source.  Decided when the int8 copy is built (ensure_blocked_copy).
    mutable bool i8_residual = true;
    mutable DevBuf d_center, d_list_scale, d_list_half, d_list_radius;
    mutable DevBuf d_row_n2i, d_row_res;
    // Tunables.  Defaults are what the dispatch rules below were measured with; every one can be set per
    // searcher through pqv_searcher_set_option (tests and benches use that to force a path) and, for the
    // profiling scripts, through a PQV_<NAME> environment variable read ONCE, when the searcher is created.
    struct Opts {
        int rerank_mode = 0;               // 0 auto, 1 stream_kernel, 2 tile path
        int tile_filter = 1;               // MFMA lower-bound screen in the batched path: 0 off, 1 by rule, 2 forced
        int filter_variant = 0;            // 1: one 16-query group per block (tile_filter_kernel)
        uint32_t cand_cap = 0;             // candidate-buffer entries per query of the wide screened path (0 = by rule: 2048, 8192 for k > 32)
        int screen_f16 = 1;                // f16 operands where possible
        int screen_i8 = 1;                 // int8 operands where possible (dim % 256 == 0)
        uint32_t seed_rows = 0;            // rows per list sampled for the thresholds (0 = by rule)
        uint32_t wide_rows = 0;            // rows per block of the wide kernel (0 = by rule)
        uint32_t tile_rows = 0;            // rows per block of the exact tile kernel (0 = 1536)
        int running_thr = 1;               // running thresholds of the wide kernel
        int defer = 1;                     // wide kernel, k > 64: survivors are appended with their bounds, evaluated after the filter (0: in it)
        int quad_xcd = -1;                 // quad-to-XCD affinity of the wide kernels (-1 = by rule)
        int single_bucket = 1;             // one query: the probe merge writes the bucketing, no pair-sort launches
        int seed_refine = 1;               // exact distances behind the k selected seed bounds tighten the first threshold (k <= 16)
        int item_grid = 1;                 // wide filter kernel: 1-D grid over (quad, existing row chunk) items
        int chunk_major = 1;               // ... numbered chunk-major (row chunk 0 of every quad first)
        int wide_waves = 0;                // waves per block of the wide kernel: 0 by rule, 4 or 8
        int probe_rows = 1;                // batched centroid probe (probe_rows_kernel) when dim % 4 == 0; 0 = stream_kernel
        int probe_screen = 1;              // ... screened on the matrix cores (probe_screen_kernel + probe_resolve_kernel): 1 by rule, 0 off,
                                           // 2 = every batch the kernels support
        uint32_t quad_width = 0;           // queries per quad of the wide kernel (0 = by rule)
        uint32_t min_blocks = 0;           // wide kernel: blocks a launch should at least have before rows per block shrink (0 = by rule)
        int pair_prune = 1;                // int8 path: drop (query, list) pairs whose centre-distance bound exceeds the query's threshold
        int i8_form = 0;                   // int8 images: 0 by rule (per-list residual where the lists are tight), 1 one centre, 2 residual
        int xcd_items = 1;                 // PairSortArgs::xcd_items (PQV_XCD_ITEMS)
        int pf96 = 1;                      // TileArgs::opt_pf96 (PQV_PF96)
        int static_dim = 1;                // TileArgs::static_dim (PQV_STATIC_DIM): 0 = the run-time row length in every screen instance
        int drain_min = 0;                 // TileArgs::drain_min (PQV_DRAIN_MIN)
        int fork_wide = 0;                 // the wide-quad launch on the lane's side stream, beside the regular instance (PQV_FORK_WIDE)
        int wide_quads = 1;                // int8, 96-query quads: lists probed by 97..160 queries of the batch take ONE 160-query quad
                                           // (8-wave blocks on 32-row tiles) instead of two passes; 0 = off
        uint32_t wide_quad_rows = 0;       // rows per block of that instance (0 = by rule: 6144)
        uint32_t partition_blocks = 0;     // pqv_topk_partition: blocks per query of partition_stream_kernel (0 = by rule; PQV_PARTITION_BLOCKS)
        uint64_t partition_range_bytes = 0;    // pqv_range_search_partition: the hit segments' byte budget of one group (0 = 1 GiB; PQV_PARTITION_RANGE_BYTES)
        int list_once = 0;                 // round 6: 1 = lists probed by more than 96 queries of the batch go to list_filter_kernel (rows stationary in
                                           // registers, ALL the list's pairs streamed past them: every such list is read once -- and measured SLOWER than
                                           // the wide-quad instance / regular quads sharing an L2: C3 2.18 against 1.87 ms of kernels, the mixture 3.7
                                           // against 2.1; DESIGN 5.4d has the counters); 0 (default) = the wide-quad instance
    };
    mutable Opts opt;
    // table searchers (pqv_table_searcher_create): n_files > 0, the index is the files' indexes concatenated -- file f owns the
    // global centroids [seg_off[f], seg_off[f + 1]) and the corpus rows [row_base[f], row_base[f] + its rows); nprobe counts per file
    uint32_t n_files = 0;                  // 0: an ordinary searcher
    std::vector<uint32_t> seg_off;         // [n_files + 1]
    std::vector<uint64_t> row_base;        // [n_files]
    uint32_t seg_max_kc = 0;               // largest file centroid count
    bool rr_cap = false;                   // PQV_TABLE_CAP_ROUND_ROBIN: max_candidates is dealt out round robin over the files
    DevBuf d_seg_off, d_seg_off64;         // seg_off on the device: u32 (merge_probe_seg_kernel), u64 (the per-file stream_kernel probe)
    mutable pqv_counters_t counters{};
    // timing
    mutable bool timing = false;
    mutable std::vector<hipEvent_t> ev;    // triples: probe-start, rerank-start, rerank-stop, end
    // PQV_COSINE (pqv.h): an ordinary searcher of the same layout over the normalised column -- n(c) centroids, the same lists, n(x)
    // rows in cos_corpus -- made under `mu` by the first cosine call or at creation (PQV_PREPARE_COSINE; ensure_cosine).  Cosine calls
    // normalise their queries and run the L2 path on it with the distances halved at the write-out.  Declared in this order: the
    // searcher goes before the corpus it borrows.
    mutable std::unique_ptr<pqv_corpus> cos_corpus;    // row-order n(x) (its rows released where `cos` keeps an IVF-ordered copy)
    mutable std::unique_ptr<pqv_searcher> cos;
    // pqv_topk_rows / pqv_score_rows: row -> list position, u32 [corpus rows], 0xFFFFFFFF for a row of no list -- made under `mu` by
    // the first candidate-list call (ensure_row_map).  List positions are the same in every layout and in `cos`: one map serves all.
    mutable DevBuf d_row_map;
    mutable uint64_t row_map_len = 0;
    mutable bool row_map_done = false;
    ~pqv_searcher();
};
pqv_searcher::~pqv_searcher() {
    if (d_ps_stats.p) {       // PQV_PROBE_SCREEN_STATS=1: what the screened probe left to the exact chains, over the searcher's life
        unsigned long long h[3] = {0, 0, 0};
        if (hipDeviceSynchronize() == hipSuccess && hipMemcpy(h, d_ps_stats.p, sizeof h, hipMemcpyDeviceToHost) == hipSuccess)
            std::fprintf(stderr, "[pqv] screened probe: %llu queries, %.2f exact evaluations per query of %u centroids, %llu all-exact queries\n",
                         h[0], h[0] ? static_cast<double>(h[1]) / static_cast<double>(h[0]) : 0.0, n_clusters, h[2]);
    }
    for (auto e : ev) (void)hipEventDestroy(e);
    pool_put(device, stream);          // (back to the device's pool: see StreamPool)
}

// The scratch lane of a call on `stream`: the lane that stream used last, else a free one, else the least
// recently assigned one.  Resolved ONCE per public entry point (under s->mu) and handed down: a lane taken
// over from another stream is first ordered behind that stream's last call (its `done` event), and
// release() records the new owner when the call's last kernel has been enqueued.  The destructor records `done` on EVERY other
// way out of an entry point: an error return half-way through a call has enqueued work on `stream` that the lane's next owner
// must still be ordered behind.
struct Lane {
    Scratch *sc = nullptr;
    hipStream_t stream = nullptr;
    Lane() = default;
    Lane(const Lane &) = delete;
    Lane &operator=(const Lane &) = delete;
    ~Lane() { if (sc && sc->done) (void)hipEventRecord(sc->done, stream); }
    int acquire(const pqv_searcher *s, hipStream_t st) {
        Scratch *l = nullptr;
        for (auto &c : s->lanes) if (c.used && c.stream == st) { l = &c; break; }
        if (!l) for (auto &c : s->lanes) if (!c.used) { l = &c; break; }
        if (!l) l = &s->lanes[s->lane_rr++ % PQV_LANES];     // only an eviction advances the cursor
        if (!l->done) HIP_TRY(hipEventCreateWithFlags(&l->done, hipEventDisableTiming));
        if (l->used && l->stream != st) HIP_TRY(hipStreamWaitEvent(st, l->done, 0));
        // owned by `st` from here on, also if the call fails half-way: whatever it enqueued runs on `st`
        l->stream = st; l->used = true;
        sc = l; stream = st;
        return PQV_OK;
    }
    // the success path's last step: the same record, checked
    int release() {
        Scratch *l = sc;
        sc = nullptr;
        HIP_TRY(hipEventRecord(l->done, stream));
        return PQV_OK;
    }
    Scratch &operator*() const { return *sc; }
    Scratch *operator->() const { return sc; }
};

// A row mask (pqv.h: pqv_row_mask): one allow bit per row of the searcher's corpus, kept as the device bitset over LIST POSITIONS
// that masked_stream_kernel reads (kernels_mask.hip) and as the caller's bytes in row order for the host replays.  The bitset is
// indexed through d_ids -- list position -> the row a call reports, the same table in every layout -- and the cosine searcher
// (ensure_cosine) shares its searcher's lists, so ONE image serves the row-order, IVF-ordered, images-only and cosine layouts.
// Immutable after creation; it holds no pointer into its searcher that it follows (owner / owner_uid are compared, never read
// through), so mask and searcher may be freed in either order.
struct pqv_row_mask {
    const pqv_searcher *owner = nullptr;
    uint64_t owner_uid = 0;
    int device = 0;
    uint64_t n_rows = 0, count = 0;
    DevBuf d_bits;                     // [ceil(n / 64) + 1] u64 image, then one u64: the allowed total
    DevBuf d_rowbits;                  // [ceil(n_rows / 64)] u64 ROW IMAGE (kernels.h): what a MASK leaf and pqv_row_mask_to_bytes read
    // [n_rows] allow bytes in row order for the host replays: a byte-made mask's are the caller's, copied at creation; a predicate
    // mask's are made from the row image by the first replay that needs them (mask_host_bytes), under host_mu
    mutable std::mutex host_mu;
    mutable std::vector<uint8_t> host;
    mutable std::atomic<bool> host_ready{false};
};
// A key column laid out for one searcher (pqv.h: pqv_row_keys): the column's values in LIST POSITION order at their own width,
// padded by a whole 64-position window, and -- where the column has validity bytes -- a position bitset in a mask's format
// (kernels.h: launch_key_layout).  Indexed through d_ids like a mask's image, so one image serves every layout, the cosine
// searcher and table searchers.  Immutable; owner / owner_uid are compared, never read through.
struct pqv_row_keys {
    const pqv_searcher *owner = nullptr;
    uint64_t owner_uid = 0;
    int device = 0;
    int dtype = 0;                     // PQV_COL_I32 / PQV_COL_I64
    uint64_t n_rows = 0, n_pos = 0;
    bool has_valid = false;
    DevBuf d_key_pos;                  // [n_words * 64] i32 / i64, n_words = ceil(n_pos / 64) + 1
    DevBuf d_valid_pos;                // [n_words] u64 (has_valid)
    // the keys in ROW order for the host replays: made from the position image by the first replay that needs them
    // (keys_host_rows), under host_mu
    mutable std::mutex host_mu;
    mutable std::vector<int64_t> host_vals;      // [n_rows], widened
    mutable std::vector<uint8_t> host_valid;     // [n_rows] (has_valid)
    mutable std::atomic<bool> host_ready{false};
    uint32_t elem_size() const { return dtype == PQV_COL_I32 ? 4u : 8u; }
    const uint64_t *valid_image() const { return has_valid ? d_valid_pos.as<uint64_t>() : nullptr; }
};
// What a search call carries beside its queries (nullptr: the plain call), in three independent parts.  The *_view functions fill
// it; the host bodies point a copy at each sub-batch's device arguments.
struct RowSelection {                  // which rows a query may return
    const uint64_t *bits;              // device image of the call's shared row mask, or nullptr
    const pqv_row_mask *mask;          // (the row-order bytes are fetched at the replay site: mask_host_bytes)
    const pqv_row_keys *keys;          // the key column of a per-query key filter, else nullptr
    uint32_t kind;                     // PQV_KEY_RANGE / PQV_KEY_IN; 0: PQV_KEY_EQ, which travels as the query-key arrays below, not as a / b
    const int64_t *h_qkeys;            // EQ, host form: [nq] query keys, indexed like the call's queries
    const int64_t *d_qkeys;            // EQ, device: the keys of the queries the kernels see (the current sub-batch's)
    const void *h_a, *h_b;             // RANGE / IN, host a / b, indexed like the call's queries (IN: lims [nq + 1] and the values)
    const void *d_a, *d_b;             // device: a / b of the queries the kernels see (IN: lims rebased to the current sub-batch)
};
struct Grouping {                      // a distinct / grouped call
    const pqv_row_keys *col;           // the group column, else nullptr
    uint32_t size;                     // pqv_topk_grouped: rows per group, >= 1 (the call's row_idx / dist are [nq, k, size]); 0: not grouped
    int64_t *d_keys;                   // where the fold writes the group values [nq * k] (device), or nullptr
    uint32_t *d_rows;                  // grouped: where the rows per group go [nq * k] (device), or nullptr
};
enum DepthSource : uint32_t { DEPTH_COUNTED = 0, DEPTH_GIVEN, DEPTH_RATIO };
struct Expansion {                     // a call with per-query probe depths (pqv_topk_expand, pqv_topk_depth)
    uint32_t max_nprobe;               // the lists the probe ranks per query, >= the call's nprobe; 0: not expanding
    // where a query's depth comes from: the passing rows or groups counted on the way (pqv_topk_expand and its grouped forms), the
    // caller's array, or the probe distances against d2_ratio times the nearest one (pqv_topk_depth: no filter, the plain call's plan)
    uint32_t source;
    float d2_ratio;
    const uint32_t *h_depths;          // GIVEN, host form: [nq], indexed like the call's queries
    const uint32_t *d_depths;          // GIVEN, device: the depths of the queries the kernels see (the current sub-batch's)
    uint32_t *d_used;                  // where the lists each query used go [nq] (device), or nullptr (the lane's scratch)
    uint32_t *h_used;                  // host form: the caller's [nq], or nullptr
};
struct SearchRequest {
    RowSelection rows;
    Grouping groups;
    Expansion expand;
    bool filtered() const { return rows.keys != nullptr; }                 // a per-query key filter of any kind ...
    bool eq_keys() const { return rows.keys && !rows.kind; }               // ... of kind PQV_KEY_EQ
    bool distinct() const { return groups.col != nullptr; }
    bool expanding() const { return expand.max_nprobe != 0; }
    // pqv_topk_depth: nothing but depths -- the plain call's kernels under per-query rank limits, not the filtered stream
    bool depth_only() const { return expanding() && expand.source != DEPTH_COUNTED; }
    // a filtered call's per-query arguments as the kernels read them
    const void *d_filter_a() const { return rows.kind ? rows.d_a : rows.d_qkeys; }
    const void *d_filter_b() const { return rows.kind ? rows.d_b : nullptr; }
};
// the lists the probe of a call ranks per query: an expanding call's max_nprobe, else its nprobe
static inline uint32_t probe_arg(const SearchRequest *mv, uint32_t nprobe) { return mv && mv->expanding() ? mv->expand.max_nprobe : nprobe; }
// a request whose rows are filtered or grouped takes the exact stream (plan_topk); one that only carries depths keeps the plain plan
static inline bool stream_request(const SearchRequest *mv) { return mv && !mv->depth_only(); }
// a mask's row image, downloaded (n_rows / 8 bytes) and expanded to one 0 / 1 byte per row
static int row_image_to_bytes(const pqv_row_mask *m, uint8_t *dst) {
    const uint64_t n_words = (m->n_rows + 63) / 64;
    std::vector<uint64_t> words;
    try { words.resize(n_words); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
    HIP_TRY(hipSetDevice(m->device));
    if (n_words) HIP_TRY(hipMemcpy(words.data(), m->d_rowbits.p, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint64_t r = 0; r < m->n_rows; ++r) dst[r] = static_cast<uint8_t>((words[r >> 6] >> (r & 63u)) & 1ull);
    return PQV_OK;
}
// The row-order allow bytes of a masked call's mask (nullptr for an unmasked call).  A predicate mask downloads its row image
// (n_rows / 8 bytes) once and expands it on the host; threads that arrive together wait for the first.  The row image was complete
// when the mask's creation returned, so the copy orders behind nothing.
static int mask_host_bytes(const SearchRequest *mv, const uint8_t **out) {
    *out = nullptr;
    if (!mv || !mv->rows.mask) return PQV_OK;
    const pqv_row_mask *m = mv->rows.mask;
    if (!m->host_ready.load(std::memory_order_acquire)) {
        std::lock_guard<std::mutex> lock(m->host_mu);
        if (!m->host_ready.load(std::memory_order_relaxed)) {
            try { m->host.resize(m->n_rows); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
            if (int rc = row_image_to_bytes(m, m->host.data())) return rc;
            m->host_ready.store(true, std::memory_order_release);
        }
    }
    *out = m->host.data();
    return PQV_OK;
}
// The row-order keys of a keyed call: the position image downloaded once (4 or 8 bytes per list position, n / 8 of validity) and
// scattered back through the searcher's host lists; threads that arrive together wait for the first.  The image was complete
// when pqv_row_keys_create returned.  `s`: the call's searcher (the keys' owner, or its cosine searcher -- the same lists).
static int keys_host_rows(const pqv_searcher *s, const pqv_row_keys *kk) {
    if (kk->host_ready.load(std::memory_order_acquire)) return PQV_OK;
    std::lock_guard<std::mutex> lock(kk->host_mu);
    if (kk->host_ready.load(std::memory_order_relaxed)) return PQV_OK;
    const std::vector<uint32_t> *h_rows = s->h_rows->get();
    if (!h_rows) return PQV_ERR_HIP;
    const uint64_t n_pos = std::min<uint64_t>(kk->n_pos, h_rows->size());
    const size_t es = kk->elem_size();
    std::vector<uint8_t> pos_vals;
    std::vector<uint64_t> pos_valid;
    try {
        pos_vals.resize(n_pos * es);
        if (kk->has_valid) pos_valid.resize((n_pos + 63) / 64);
        kk->host_vals.assign(kk->n_rows, 0);
        if (kk->has_valid) kk->host_valid.assign(kk->n_rows, 0);
    } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
    HIP_TRY(hipSetDevice(kk->device));
    if (n_pos) HIP_TRY(hipMemcpy(pos_vals.data(), kk->d_key_pos.p, n_pos * es, hipMemcpyDeviceToHost));
    if (!pos_valid.empty()) HIP_TRY(hipMemcpy(pos_valid.data(), kk->d_valid_pos.p, pos_valid.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
    for (uint64_t p = 0; p < n_pos; ++p) {
        const uint32_t r = (*h_rows)[p];
        if (r >= kk->n_rows) continue;
        if (es == 4) { int32_t v; std::memcpy(&v, pos_vals.data() + p * 4, 4); kk->host_vals[r] = v; }
        else std::memcpy(&kk->host_vals[r], pos_vals.data() + p * 8, 8);
        if (kk->has_valid) kk->host_valid[r] = static_cast<uint8_t>((pos_valid[p >> 6] >> (p & 63u)) & 1ull);
    }
    kk->host_ready.store(true, std::memory_order_release);
    return PQV_OK;
}
// The allow test of a host replay: the mask's row-order bytes and / or a keyed call's M_q (pqv.h) for the query at index `q` of
// the call's batch.  Unset (an unfiltered call): every row passes.
struct RowFilter {
    const uint8_t *allow = nullptr;
    const int64_t *key_vals = nullptr;
    const uint8_t *key_valid = nullptr;
    int64_t qkey = 0;                              // EQ: the key; RANGE: the lower bound
    uint32_t kind = PQV_KEY_EQ;
    int64_t qhi = 0;                               // RANGE: the upper bound
    const int64_t *set_beg = nullptr, *set_end = nullptr;      // IN: the query's slice, strictly ascending
    bool active() const { return allow || key_vals; }
    bool pass(uint32_t row) const {
        if (allow && !allow[row]) return false;
        if (key_vals) {
            if (key_valid && !key_valid[row]) return false;
            const int64_t v = key_vals[row];
            if (kind == PQV_KEY_EQ) return v == qkey;
            if (kind == PQV_KEY_RANGE) return qkey <= v && v <= qhi;
            return std::binary_search(set_beg, set_end, v);
        }
        return true;
    }
};
static int row_filter(const pqv_searcher *s, const SearchRequest *mv, uint64_t q, RowFilter &f) {
    f = RowFilter{};
    if (!mv) return PQV_OK;
    if (int rc = mask_host_bytes(mv, &f.allow)) return rc;
    if (mv->rows.keys) {
        if (int rc = keys_host_rows(s, mv->rows.keys)) return rc;
        f.key_vals = mv->rows.keys->host_vals.data();
        f.key_valid = mv->rows.keys->has_valid ? mv->rows.keys->host_valid.data() : nullptr;
        f.kind = mv->rows.kind;
        if (mv->rows.kind == PQV_KEY_RANGE) {
            f.qkey = static_cast<const int64_t *>(mv->rows.h_a)[q];
            f.qhi = static_cast<const int64_t *>(mv->rows.h_b)[q];
        } else if (mv->rows.kind == PQV_KEY_IN) {
            const uint64_t *lims = static_cast<const uint64_t *>(mv->rows.h_a);
            f.set_beg = static_cast<const int64_t *>(mv->rows.h_b) + lims[q];
            f.set_end = static_cast<const int64_t *>(mv->rows.h_b) + lims[q + 1];
        } else {
            f.qkey = mv->rows.h_qkeys[q];
        }
    }
    return PQV_OK;
}
// The RANGE / IN arrays of a filter descriptor for the sub-batch [q0, q0 + b): uploaded on `st` into the lane's scratch, *d_a / *d_b
// pointed at them.  `lims` keeps an IN filter's rebased offsets alive until the sub-batch's synchronisation.
// SLICE_ROWS: RowSelection::kind of a candidate-list call (pqv_topk_rows), beside pqv.h's PQV_KEY_* -- a = lims, b = u32 row ids.
constexpr uint32_t SLICE_ROWS = 3;
static int upload_filter_arrays(Scratch &sc, uint32_t kind, const void *h_a, const void *h_b, uint32_t q0, uint32_t b, std::vector<uint64_t> &lims,
                                hipStream_t st, const void **d_a, const void **d_b) {
    if (kind == PQV_KEY_RANGE) {
        HIP_TRY(sc.s_qfilt_a.ensure(static_cast<size_t>(b) * sizeof(int64_t)));
        HIP_TRY(sc.s_qfilt_b.ensure(static_cast<size_t>(b) * sizeof(int64_t)));
        HIP_TRY(hipMemcpyAsync(sc.s_qfilt_a.p, static_cast<const int64_t *>(h_a) + q0, static_cast<size_t>(b) * sizeof(int64_t), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(sc.s_qfilt_b.p, static_cast<const int64_t *>(h_b) + q0, static_cast<size_t>(b) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    } else {
        // (PQV_KEY_IN's i64 values, or -- SLICE_ROWS -- a candidate-list call's u32 row ids: lims + slices either way)
        const size_t vs = kind == SLICE_ROWS ? sizeof(uint32_t) : sizeof(int64_t);
        const uint64_t *hl = static_cast<const uint64_t *>(h_a);
        const uint64_t base = hl[q0], n_vals = hl[q0 + b] - base;
        try { lims.resize(static_cast<size_t>(b) + 1); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
        for (uint32_t i = 0; i <= b; ++i) lims[i] = hl[q0 + i] - base;
        HIP_TRY(sc.s_qfilt_a.ensure((static_cast<size_t>(b) + 1) * sizeof(uint64_t)));
        HIP_TRY(sc.s_qfilt_b.ensure(static_cast<size_t>(n_vals) * vs));
        HIP_TRY(hipMemcpyAsync(sc.s_qfilt_a.p, lims.data(), (static_cast<size_t>(b) + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        if (n_vals)
            HIP_TRY(hipMemcpyAsync(sc.s_qfilt_b.p, static_cast<const char *>(h_b) + base * vs, static_cast<size_t>(n_vals) * vs, hipMemcpyHostToDevice, st));
    }
    *d_a = sc.s_qfilt_a.p; *d_b = sc.s_qfilt_b.p;
    return PQV_OK;
}
// A host call's per-query filter arguments (rq's host arrays; a call without them: nothing to do) for the sub-batch [q0, q0 + b):
// uploaded on `st` into the lane's scratch, `sub` pointed at them.
static int upload_query_filter(Scratch &sc, const SearchRequest *rq, SearchRequest &sub, uint32_t q0, uint32_t b, std::vector<uint64_t> &lims,
                               hipStream_t st) {
    if (!rq) return PQV_OK;
    if (rq->rows.kind) return upload_filter_arrays(sc, rq->rows.kind, rq->rows.h_a, rq->rows.h_b, q0, b, lims, st, &sub.rows.d_a, &sub.rows.d_b);
    if (!rq->rows.h_qkeys) return PQV_OK;
    HIP_TRY(sc.s_qkeys.ensure(static_cast<size_t>(b) * sizeof(int64_t)));
    HIP_TRY(hipMemcpyAsync(sc.s_qkeys.p, rq->rows.h_qkeys + q0, static_cast<size_t>(b) * sizeof(int64_t), hipMemcpyHostToDevice, st));
    sub.rows.d_qkeys = sc.s_qkeys.as<int64_t>();
    return PQV_OK;
}
// the per-query filter of a distinct / grouped call that has one (mv->filtered() beside mv->distinct()), as its kernels read it
static pqv::GroupFilterArgs group_filter_args(const SearchRequest *mv) {
    const pqv_row_keys *kk = mv->rows.keys;
    return pqv::GroupFilterArgs{kk->d_key_pos.p, kk->valid_image(), kk->elem_size(), mv->rows.kind, mv->d_filter_a(), mv->d_filter_b()};
}
// The STREAM_TOPK / STREAM_RANGE pass of any call: the plain one (rq == nullptr; stats and n_cand unused: the probe merge counts),
// PQV_DOT, masked, keyed / filtered, and distinct (STREAM_TOPK only, the per-wave lists' group values go to part_grp)
static hipError_t launch_stream_pass(const pqv::StreamArgs &ra, const SearchRequest *rq, unsigned long long *stats, const uint64_t *n_cand,
                                     pqv::StreamMode mode, hipStream_t stream, int64_t *part_grp = nullptr,
                                     const uint32_t *rank_limit = nullptr) {
    if (!rq) return ra.metric == PQV_DOT ? pqv::launch_dot_stream(ra, nullptr, mode, stream) : pqv::launch_stream(ra, mode, stream);
    if (rq->distinct()) {
        if (mode != pqv::STREAM_TOPK) return hipErrorInvalidValue;
        const pqv_row_keys *gk = rq->groups.col;
        const pqv::DistinctArgs da{rq->rows.bits, stats, n_cand, gk->d_key_pos.p, gk->valid_image(), gk->elem_size(), part_grp, rank_limit};
        if (rq->filtered()) return pqv::launch_distinct_filter_stream(ra, da, group_filter_args(rq), stream);
        return pqv::launch_distinct_stream(ra, da, stream);
    }
    if (rq->filtered()) {
        const pqv_row_keys *kk = rq->rows.keys;
        const pqv::KeyedArgs ka{rq->rows.bits, stats, n_cand, kk->d_key_pos.p, kk->valid_image(), rq->rows.d_qkeys, kk->elem_size(), rank_limit};
        if (rq->rows.kind) {
            pqv::KeyFilterArgs fa{};
            static_cast<pqv::KeyedArgs &>(fa) = ka;
            fa.kind = rq->rows.kind; fa.a = rq->rows.d_a; fa.b = rq->rows.d_b;
            return pqv::launch_key_filter_stream(ra, fa, mode, stream);
        }
        return pqv::launch_keyed_stream(ra, ka, mode, stream);
    }
    const pqv::MaskedArgs ma{rq->rows.bits, stats, n_cand, rank_limit};
    if (ra.metric == PQV_DOT) return pqv::launch_dot_stream(ra, &ma, mode, stream);
    return pqv::launch_masked_stream(ra, ma, mode, stream);
}

// ---------------------------------------------------------------------------------------
// misc
// ---------------------------------------------------------------------------------------
extern "C" const char *pqv_last_error(void) { return g_last_error.c_str(); }

extern "C" int pqv_device_count(void) {
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) return 0;
    return count < 0 ? 0 : count;
}

extern "C" int pqv_abi_version(void) { return 101; }

extern "C" int pqv_diag_rng(const uint8_t *seed32, uint64_t seed64, int mode, uint64_t arg, uint64_t *out, uint64_t n) {
    return guard([&] {
        if (!out && n) return fail(PQV_ERR_INVALID, "out must not be NULL");
        pqv::StdRng rng = seed32 ? pqv::StdRng::from_seed(seed32) : pqv::StdRng::seed_from_u64(seed64);
        if (mode == 4) {
            if (n > arg) return fail(PQV_ERR_INVALID, "amount exceeds length");
            const std::vector<uint64_t> s = pqv::index_sample(rng, arg, n);
            for (uint64_t i = 0; i < n; ++i) out[i] = s[i];
            return static_cast<int>(PQV_OK);
        }
        for (uint64_t i = 0; i < n; ++i) {
            if (mode == 0) out[i] = rng.next_u64();
            else if (mode == 1) out[i] = rng.next_u32();
            else if (mode == 2) out[i] = rng.range_usize(0, arg);
            else if (mode == 3) { const float f = rng.unit_f32(); uint32_t b; std::memcpy(&b, &f, 4); out[i] = b; }
            else return fail(PQV_ERR_INVALID, "unknown mode");
        }
        return static_cast<int>(PQV_OK);
    });
}

// ---------------------------------------------------------------------------------------
// corpus
// ---------------------------------------------------------------------------------------
static int pqv_corpus_create_impl(int device, uint64_t capacity_rows, uint32_t dim,
                                 pqv_corpus **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");  // mod.rs:59
    if (capacity_rows > 0xFFFFFFFFull)
        return fail(PQV_ERR_UNSUPPORTED, "row ids are u32: at most 4294967295 rows per corpus");
    if (int rc = use_device(device)) return rc;
    pqv_corpus *c = new (std::nothrow) pqv_corpus();
    if (!c) return fail(PQV_ERR_OOM, "host allocation failed");
    c->device = device;
    c->dim = dim;
    c->capacity = capacity_rows;
    const size_t bytes = std::max<size_t>(16, static_cast<size_t>(capacity_rows) * dim * sizeof(float));
    hipError_t e = hipMalloc(reinterpret_cast<void **>(&c->d_rows), bytes);
    if (e != hipSuccess) {
        delete c;
        return fail(PQV_ERR_OOM, std::string("hipMalloc(corpus): ") + hipGetErrorString(e));
    }
    e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(PQV_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    (void)pqv::touch_build(c->stream);            // (the stream's hardware queue is set up by its first launch: here, not in the build)
    (void)hipStreamSynchronize(c->stream);
    *out = c;
    return PQV_OK;
}
extern "C" int pqv_corpus_create(int device, uint64_t capacity_rows, uint32_t dim,
                                 pqv_corpus **out) {
    return guard([&] { return pqv_corpus_create_impl(device, capacity_rows, dim, out); });
}

static int pqv_corpus_append_impl(pqv_corpus *c, const float *rows, uint64_t n_rows) {
    if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
    if (!c->owned) return fail(PQV_ERR_INVALID, "cannot append to a borrowed device buffer");
    if (n_rows == 0) return PQV_OK;
    if (!rows) return fail(PQV_ERR_INVALID, "rows must not be NULL");
    if (c->n + n_rows > c->capacity) return fail(PQV_ERR_INVALID, "corpus capacity exceeded");
    if (int rc = use_device(c->device)) return rc;
    HIP_TRY(hipMemcpy(c->d_rows + c->n * c->dim, rows, static_cast<size_t>(n_rows) * c->dim * sizeof(float),
                      hipMemcpyHostToDevice));
    c->n += n_rows;
    return PQV_OK;
}
extern "C" int pqv_corpus_append(pqv_corpus *c, const float *rows, uint64_t n_rows) {
    return guard([&] { return pqv_corpus_append_impl(c, rows, n_rows); });
}

static int pqv_corpus_append_f64_impl(pqv_corpus *c, const double *rows, uint64_t n_rows) {
    if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
    if (!c->owned) return fail(PQV_ERR_INVALID, "cannot append to a borrowed device buffer");
    if (n_rows == 0) return PQV_OK;
    if (!rows) return fail(PQV_ERR_INVALID, "rows must not be NULL");
    if (c->n + n_rows > c->capacity) return fail(PQV_ERR_INVALID, "corpus capacity exceeded");
    if (int rc = use_device(c->device)) return rc;
    const uint64_t count = n_rows * c->dim;
    DevBuf stage;
    HIP_TRY(stage.alloc(count * sizeof(double)));
    HIP_TRY(hipMemcpy(stage.p, rows, count * sizeof(double), hipMemcpyHostToDevice));
    HIP_TRY(pqv::launch_narrow_f64(stage.as<double>(), count, c->d_rows + c->n * c->dim, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->n += n_rows;
    return PQV_OK;
}
extern "C" int pqv_corpus_append_f64(pqv_corpus *c, const double *rows, uint64_t n_rows) {
    return guard([&] { return pqv_corpus_append_f64_impl(c, rows, n_rows); });
}

// ---- streaming upload (N1) ----------------------------------------------------------------
namespace {
int upload_stage_of(pqv_corpus *c, UploadStage **out) {
    std::lock_guard<std::mutex> lock(c->upload_mu);
    if (!c->upload) {
        std::unique_ptr<UploadStage> u(new UploadStage());
        for (int i = 0; i < UploadStage::NS; ++i) HIP_TRY(hipStreamCreateWithFlags(&u->copy_stream[i], hipStreamNonBlocking));
        for (int i = 0; i < UploadStage::N; ++i) {
            HIP_TRY(hipHostMalloc(&u->pin[i], UploadStage::BYTES, hipHostMallocDefault));
            HIP_TRY(hipEventCreateWithFlags(&u->ev[i], hipEventDisableTiming));
        }
        c->upload = std::move(u);
    }
    *out = c->upload.get();
    return PQV_OK;
}
// a staging buffer nobody else is filling: a free one, else the in-flight one whose DMA ends first (waited for outside the lock)
int upload_claim(UploadStage *u, int *slot) {
    std::unique_lock<std::mutex> lock(u->mu);
    for (;;) {
        for (int i = 0; i < UploadStage::N; ++i) if (u->state[i] == 0) { u->state[i] = 1; *slot = i; return PQV_OK; }
        for (int i = 0; i < UploadStage::N; ++i)
            if (u->state[i] == 2) {
                u->state[i] = 1;                       // ours; its previous DMA still has to finish
                lock.unlock();
                const hipError_t e = hipEventSynchronize(u->ev[i]);
                if (e != hipSuccess) { lock.lock(); u->state[i] = 0; u->cv.notify_one(); lock.unlock(); HIP_TRY(e); }
                *slot = i;
                return PQV_OK;
            }
        u->cv.wait(lock);                              // every buffer is being filled by another thread
    }
}
void upload_release(UploadStage *u, int slot, bool in_flight) {
    { std::lock_guard<std::mutex> lock(u->mu); u->state[slot] = in_flight ? 2 : 0; }
    u->cv.notify_one();
}
template <class T>
int corpus_write_rows(pqv_corpus *c, uint64_t row_offset, const T *rows, uint64_t n_rows) {
    if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
    if (!c->owned) return fail(PQV_ERR_INVALID, "cannot write into a borrowed device buffer");
    if (n_rows == 0) return PQV_OK;
    if (!rows) return fail(PQV_ERR_INVALID, "rows must not be NULL");
    if (row_offset > c->capacity || n_rows > c->capacity - row_offset) return fail(PQV_ERR_INVALID, "corpus capacity exceeded");
    if (int rc = use_device(c->device)) return rc;
    UploadStage *u = nullptr;
    if (int rc = upload_stage_of(c, &u)) return rc;
    const uint64_t row_bytes = static_cast<uint64_t>(c->dim) * sizeof(T);
    const uint64_t rows_per_piece = std::max<uint64_t>(1, UploadStage::BYTES / row_bytes);
    if (row_bytes > UploadStage::BYTES) return fail(PQV_ERR_INVALID, "a row exceeds the staging buffer");
    for (uint64_t r0 = 0; r0 < n_rows; r0 += rows_per_piece) {
        const uint64_t m = std::min<uint64_t>(rows_per_piece, n_rows - r0);
        int slot = -1;
        if (int rc = upload_claim(u, &slot)) return rc;
        std::memcpy(u->pin[slot], rows + r0 * c->dim, m * row_bytes);
        hipStream_t cs = u->copy_stream[slot % UploadStage::NS];
        float *dst = c->d_rows + (row_offset + r0) * c->dim;
        hipError_t e = hipSuccess;
        if (std::is_same<T, float>::value) {
            e = hipMemcpyAsync(dst, u->pin[slot], m * row_bytes, hipMemcpyHostToDevice, cs);
        } else {
            if (!u->dev64[slot]) e = hipMalloc(&u->dev64[slot], UploadStage::BYTES);
            if (e == hipSuccess) e = hipMemcpyAsync(u->dev64[slot], u->pin[slot], m * row_bytes, hipMemcpyHostToDevice, cs);
            if (e == hipSuccess) e = pqv::launch_narrow_f64(static_cast<const double *>(u->dev64[slot]), m * c->dim, dst, cs);
        }
        if (e == hipSuccess) e = hipEventRecord(u->ev[slot], cs);
        upload_release(u, slot, e == hipSuccess);
        HIP_TRY(e);
    }
    return PQV_OK;
}
}  // namespace
extern "C" int pqv_corpus_write_rows(pqv_corpus *c, uint64_t row_offset, const float *rows, uint64_t n_rows) {
    return guard([&] { return corpus_write_rows<float>(c, row_offset, rows, n_rows); });
}
extern "C" int pqv_corpus_write_rows_f64(pqv_corpus *c, uint64_t row_offset, const double *rows, uint64_t n_rows) {
    return guard([&] { return corpus_write_rows<double>(c, row_offset, rows, n_rows); });
}
extern "C" int pqv_corpus_finish(pqv_corpus *c, uint64_t n_rows) {
    return guard([&]() -> int {
        if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
        if (n_rows > c->capacity) return fail(PQV_ERR_INVALID, "corpus capacity exceeded");
        if (int rc = use_device(c->device)) return rc;
        if (c->upload) {
            for (int i = 0; i < UploadStage::NS; ++i) HIP_TRY(hipStreamSynchronize(c->upload->copy_stream[i]));
            std::lock_guard<std::mutex> lock(c->upload_mu);
            c->upload.reset();                     // the pinned buffers go back: a resident corpus does not keep 128 MB of them
        }
        c->n = n_rows;
        return PQV_OK;
    });
}

// ---- Parquet page helpers (N1; host only) ---------------------------------------------------
namespace {
// One run of the RLE / bit-packed hybrid at a time: fn(value, count) for an RLE run, fn(values...) one by one for a bit-packed
// group.  Returns false on a malformed stream.  `want` values are consumed (a final bit-packed group may hold padding).
template <class F>
bool hybrid_runs(const uint8_t *p, uint64_t len, uint32_t bw, uint64_t want, F &&fn) {
    if (bw > 32) return false;
    const uint8_t *end = p + len;
    const uint32_t vbytes = (bw + 7) / 8;
    const uint64_t mask = bw == 32 ? 0xFFFFFFFFull : ((1ull << bw) - 1ull);
    uint64_t got = 0;
    while (got < want) {
        uint64_t h = 0;
        for (uint32_t shift = 0;; shift += 7) {
            if (p >= end || shift > 56) return false;
            const uint8_t b = *p++;
            h |= static_cast<uint64_t>(b & 0x7F) << shift;
            if (!(b & 0x80)) break;
        }
        if (h & 1) {                                     // bit-packed: (h >> 1) groups of 8 values
            // (group count checked BEFORE the multiplications: a crafted 9-byte varint would wrap nbytes to 0 and pass)
            const uint64_t groups = h >> 1;
            if (groups == 0 || groups > (1ull << 56) || (bw != 0 && groups > static_cast<uint64_t>(end - p) / bw)) return false;
            const uint64_t nvals = groups * 8, nbytes = groups * bw;
            const uint64_t use = std::min<uint64_t>(nvals, want - got);
            uint64_t acc = 0; uint32_t nb = 0; const uint8_t *q = p;
            for (uint64_t i = 0; i < use; ++i) {
                while (nb < bw) { acc |= static_cast<uint64_t>(*q++) << nb; nb += 8; }
                if (!fn(static_cast<uint32_t>(acc & mask), 1ull)) return true;       // the callback has its answer
                acc >>= bw; nb -= bw;
            }
            p += nbytes; got += use;
        } else {                                         // RLE: count, value in ceil(bw / 8) bytes
            const uint64_t cnt = h >> 1;
            if (cnt == 0 || static_cast<uint64_t>(end - p) < vbytes) return false;
            uint32_t v = 0;
            for (uint32_t i = 0; i < vbytes; ++i) v |= static_cast<uint32_t>(p[i]) << (8 * i);
            p += vbytes;
            const uint64_t use = std::min<uint64_t>(cnt, want - got);
            if (!fn(v, use)) return true;
            got += use;
        }
    }
    return true;
}
}  // namespace
extern "C" int pqv_parquet_levels_check(const uint8_t *buf, uint64_t len, uint32_t bit_width, uint64_t n_values, int mode, uint64_t expect,
                                        uint64_t *period_out) {
    return guard([&]() -> int {
        if (n_values == 0) return 0;
        if (!buf) return fail(PQV_ERR_INVALID, "buf must not be NULL");
        if (mode == 1 && expect == 0) {
            // discover the list length: the position of the second level 0 (the first must be at position 0)
            if (!period_out) return fail(PQV_ERR_INVALID, "list length must be > 0");
            uint64_t at = 0, zeros = 0, second = 0;
            const bool w0 = hybrid_runs(buf, len, bit_width, n_values, [&](uint32_t v, uint64_t cnt) {
                if (v == 0) {
                    if (zeros == 0 && at != 0) { zeros = 99; return false; }          // the page starts inside a row
                    if (zeros == 0 && cnt >= 2) { second = 1; zeros = 2; return false; }
                    if (zeros == 1) { second = at; zeros = 2; return false; }
                    zeros = 1;
                }
                at += cnt;
                return true;
            });
            if (!w0) return fail(PQV_ERR_INVALID, "malformed RLE / bit-packed level run");
            if (zeros == 99 || zeros == 0) return 1;
            expect = zeros == 2 ? second : n_values;
            *period_out = expect;
            if (expect == 0) return 1;
        }
        bool ok = true;
        uint64_t pos = 0;                                // mode 1: position inside the page, in values
        const bool well = hybrid_runs(buf, len, bit_width, n_values, [&](uint32_t v, uint64_t cnt) {
            if (mode == 0) { ok = v == expect; return ok; }
            // repetition levels: 0 exactly at the multiples of `expect`
            const uint64_t ph = pos % expect;
            if (v == 0) ok = ph == 0 && (cnt == 1 || expect == 1);
            else ok = v == 1 && ph != 0 && ph + cnt <= expect;
            pos += cnt;
            return ok;
        });
        if (!well) return fail(PQV_ERR_INVALID, "malformed RLE / bit-packed level run");
        if (ok && mode == 1 && pos % expect != 0) ok = false;     // the page ends inside a row
        return ok ? 0 : 1;
    });
}
namespace {
// (levels as above, without the error text: 0 as expected, 1 different, -1 malformed)
int levels_plain(const uint8_t *buf, uint64_t len, uint32_t bw, uint64_t n_values, int mode, uint64_t expect) {
    bool ok = true;
    uint64_t pos = 0;
    const bool well = hybrid_runs(buf, len, bw, n_values, [&](uint32_t v, uint64_t cnt) {
        if (mode == 0) { ok = v == expect; return ok; }
        const uint64_t ph = pos % expect;
        if (v == 0) ok = ph == 0 && (cnt == 1 || expect == 1);
        else ok = v == 1 && ph != 0 && ph + cnt <= expect;
        pos += cnt;
        return ok;
    });
    if (!well) return -1;
    if (ok && mode == 1 && pos % expect != 0) ok = false;
    return ok ? 0 : 1;
}
}  // namespace

// A run of uncompressed PLAIN v1 data pages of a `List<f32|f64>` leaf, straight from the mapped file: per page the two level
// runs are checked (repetition level 0 exactly every `dim` values, every definition level == max_def) and the values behind
// them are uploaded like pqv_corpus_write_rows at row first_value / dim.  One call per dozen pages keeps a Python caller's
// interpreter lock out of the loop.  Returns 0, or 1 with *bad_page = the first page that is not what the plan assumed
// (nothing of it is uploaded; the caller re-reads the column through its general reader).
extern "C" int pqv_corpus_write_plain_pages(pqv_corpus *c, const uint8_t *file_base, const uint64_t *body_off, const uint32_t *body_len,
                                            const uint64_t *first_value, const uint32_t *n_values, uint32_t n_pages, uint32_t dim,
                                            uint32_t max_def, int f64, uint32_t *bad_page) {
    return guard([&]() -> int {
        if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
        if (!file_base || !body_off || !body_len || !first_value || !n_values) return fail(PQV_ERR_INVALID, "page tables must not be NULL");
        if (dim == 0 || dim != c->dim) return fail(PQV_ERR_INVALID, "list length does not match the corpus");
        uint32_t def_bw = 0;
        for (uint32_t v = max_def; v; v >>= 1) ++def_bw;
        const uint64_t esz = f64 ? 8 : 4;
        for (uint32_t i = 0; i < n_pages; ++i) {
            const uint8_t *b = file_base + body_off[i];
            const uint64_t blen = body_len[i], nv = n_values[i];
            uint64_t p = 0;
            bool good = nv > 0 && nv % dim == 0 && first_value[i] % dim == 0;
            for (int run = 0; run < 2 && good; ++run) {
                if (p + 4 > blen) { good = false; break; }
                uint32_t n;
                std::memcpy(&n, b + p, 4);
                if (p + 4 + n > blen) { good = false; break; }
                good = levels_plain(b + p + 4, n, run == 0 ? 1u : def_bw, nv, run == 0 ? 1 : 0, run == 0 ? dim : max_def) == 0;
                p += 4 + static_cast<uint64_t>(n);
            }
            if (good && blen - p != nv * esz) good = false;
            if (!good) { if (bad_page) *bad_page = i; return 1; }
            const uint64_t row = first_value[i] / dim, rows = nv / dim;
            int rc = f64 ? corpus_write_rows<double>(c, row, reinterpret_cast<const double *>(b + p), rows)
                         : corpus_write_rows<float>(c, row, reinterpret_cast<const float *>(b + p), rows);
            if (rc != PQV_OK) return rc;
        }
        return PQV_OK;
    });
}

// ---- Thrift compact protocol, as far as a Parquet PageHeader needs it ----
namespace {
struct TcReader {
    const uint8_t *p, *end;
    bool ok = true;
    uint64_t varint() {
        uint64_t v = 0;
        for (int sh = 0; sh < 70; sh += 7) {
            if (p >= end) { ok = false; return 0; }
            const uint8_t b = *p++;
            v |= static_cast<uint64_t>(b & 0x7F) << sh;
            if (!(b & 0x80)) return v;
        }
        ok = false;
        return 0;
    }
    int64_t zigzag() { const uint64_t v = varint(); return static_cast<int64_t>(v >> 1) ^ -static_cast<int64_t>(v & 1); }
    void skip_bytes(uint64_t n) { if (n > static_cast<uint64_t>(end - p)) { ok = false; p = end; } else p += n; }
    void skip(int type, int depth) {
        if (!ok || depth > 16) { ok = false; return; }
        switch (type) {
            case 1: case 2: return;                       // bool in the field header
            case 3: skip_bytes(1); return;
            case 4: case 5: case 6: (void)varint(); return;
            case 7: skip_bytes(8); return;
            case 8: skip_bytes(varint()); return;
            case 9: case 10: {
                if (p >= end) { ok = false; return; }
                const uint8_t h = *p++;
                uint64_t n = h >> 4;
                const int et = h & 15;
                if (n == 15) n = varint();
                for (uint64_t i = 0; i < n && ok; ++i) { if (et == 1 || et == 2) skip_bytes(1); else skip(et, depth + 1); }
                return;
            }
            case 11: {
                const uint64_t n = varint();
                if (n == 0) return;
                if (p >= end) { ok = false; return; }
                const uint8_t kv = *p++;
                for (uint64_t i = 0; i < n && ok; ++i) {
                    const int kt = kv >> 4, vt = kv & 15;
                    if (kt == 1 || kt == 2) skip_bytes(1); else skip(kt, depth + 1);
                    if (vt == 1 || vt == 2) skip_bytes(1); else skip(vt, depth + 1);
                }
                return;
            }
            case 12: skip_struct(depth + 1); return;
            default: ok = false; return;
        }
    }
    // fields of a struct: f(field id, type) consumes the value and returns true, or returns false to have it skipped
    template <class F> void fields(int depth, F f) {
        int16_t last = 0;
        while (ok) {
            if (p >= end) { ok = false; return; }
            const uint8_t h = *p++;
            if (h == 0) return;
            const int type = h & 15, delta = h >> 4;
            int16_t id = delta ? static_cast<int16_t>(last + delta) : static_cast<int16_t>(zigzag());
            last = id;
            if (!f(id, type)) skip(type, depth);
        }
    }
    void skip_struct(int depth) { fields(depth, [](int16_t, int) { return false; }); }
};
}  // namespace

// Page headers of one column chunk (format/PageHeader of parquet.thrift), one after the other from `buf`: per page 8 ints
// {type, header bytes, compressed_page_size, uncompressed_page_size, num_values, encoding, definition_level_encoding,
// repetition_level_encoding} (the last four from data_page_header / dictionary_page_header; -1 where absent; v2 data pages and
// index pages report their type only).  Stops at `len`, after `max_pages`, or once `stop_values` values have been seen in data
// pages; *n_pages = pages written.  An error for a header that does not parse or a page that runs past `len`.
extern "C" int pqv_parquet_page_headers(const uint8_t *buf, uint64_t len, uint64_t stop_values, uint32_t max_pages, int32_t *out, uint32_t *n_pages) {
    return guard([&]() -> int {
        if (!buf || !out || !n_pages) return fail(PQV_ERR_INVALID, "buf, out and n_pages must not be NULL");
        uint64_t pos = 0, seen = 0;
        uint32_t n = 0;
        while (pos < len && n < max_pages && (stop_values == 0 || seen < stop_values)) {
            TcReader r{buf + pos, buf + len};
            int32_t *o = out + static_cast<size_t>(n) * 8;
            for (int i = 0; i < 8; ++i) o[i] = -1;
            r.fields(0, [&](int16_t id, int type) {
                const bool i32 = type == 4 || type == 5 || type == 6;
                if (id == 1 && i32) { o[0] = static_cast<int32_t>(r.zigzag()); return true; }
                if (id == 2 && i32) { o[3] = static_cast<int32_t>(r.zigzag()); return true; }
                if (id == 3 && i32) { o[2] = static_cast<int32_t>(r.zigzag()); return true; }
                if ((id == 5 || id == 7) && type == 12) {
                    r.fields(1, [&](int16_t id2, int type2) {
                        const bool j32 = type2 == 4 || type2 == 5 || type2 == 6;
                        if (id2 >= 1 && id2 <= (id == 5 ? 4 : 2) && j32) { o[3 + id2] = static_cast<int32_t>(r.zigzag()); return true; }
                        return false;
                    });
                    return true;
                }
                return false;
            });
            if (!r.ok) return fail(PQV_ERR_INVALID, "malformed Parquet page header");
            const uint64_t hlen = static_cast<uint64_t>(r.p - (buf + pos));
            o[1] = static_cast<int32_t>(hlen);
            if (o[0] < 0 || o[2] < 0 || o[3] < 0 || hlen + static_cast<uint64_t>(o[2]) > len - pos)
                return fail(PQV_ERR_INVALID, "Parquet page runs past its column chunk");
            if (o[0] == 0 && o[4] > 0) seen += static_cast<uint64_t>(o[4]);
            pos += hlen + static_cast<uint64_t>(o[2]);
            ++n;
        }
        *n_pages = n;
        return PQV_OK;
    });
}

extern "C" int pqv_parquet_dict_decode(const uint8_t *buf, uint64_t len, const void *dict, uint64_t dict_n, uint32_t elem_size,
                                       uint64_t n_values, void *out) {
    return guard([&]() -> int {
        if (n_values == 0) return 0;
        if (!buf || !dict || !out || len < 1 || (elem_size != 4 && elem_size != 8)) return fail(PQV_ERR_INVALID, "bad arguments");
        const uint32_t bw = buf[0];
        uint64_t at = 0;
        bool in_range = true;
        auto put = [&](uint32_t idx, uint64_t cnt) {
            if (idx >= dict_n) { in_range = false; return false; }
            if (elem_size == 4) { const uint32_t v = static_cast<const uint32_t *>(dict)[idx]; uint32_t *o = static_cast<uint32_t *>(out) + at; for (uint64_t i = 0; i < cnt; ++i) o[i] = v; }
            else { const uint64_t v = static_cast<const uint64_t *>(dict)[idx]; uint64_t *o = static_cast<uint64_t *>(out) + at; for (uint64_t i = 0; i < cnt; ++i) o[i] = v; }
            at += cnt;
            return true;
        };
        if (bw == 0) { put(0, n_values); return in_range ? 0 : fail(PQV_ERR_INVALID, "dictionary index out of range"); }
        const bool well = hybrid_runs(buf + 1, len - 1, bw, n_values, put);
        if (!well || !in_range || at != n_values) return fail(PQV_ERR_INVALID, "malformed dictionary-encoded page");
        return 0;
    });
}

static int pqv_corpus_upload_impl(int device, const float *rows, uint64_t n, uint32_t dim,
                                 pqv_corpus **out) {
    if (int rc = pqv_corpus_create(device, n, dim, out)) return rc;
    if (int rc = pqv_corpus_append(*out, rows, n)) {
        delete *out;
        *out = nullptr;
        return rc;
    }
    return PQV_OK;
}
extern "C" int pqv_corpus_upload(int device, const float *rows, uint64_t n, uint32_t dim,
                                 pqv_corpus **out) {
    return guard([&] { return pqv_corpus_upload_impl(device, rows, n, dim, out); });
}

static int pqv_corpus_from_device_impl(int device, const void *d_rows, uint64_t n, uint32_t dim,
                                      pqv_corpus **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");
    if (n > 0xFFFFFFFFull)
        return fail(PQV_ERR_UNSUPPORTED, "row ids are u32: at most 4294967295 rows per corpus");
    if (n && !d_rows) return fail(PQV_ERR_INVALID, "d_rows must not be NULL");
    if (int rc = use_device(device)) return rc;
    pqv_corpus *c = new (std::nothrow) pqv_corpus();
    if (!c) return fail(PQV_ERR_OOM, "host allocation failed");
    c->device = device; c->dim = dim; c->n = n; c->capacity = n;
    c->d_rows = const_cast<float *>(static_cast<const float *>(d_rows));
    c->owned = false;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
        delete c;
        return fail(PQV_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e));
    }
    (void)pqv::touch_build(c->stream);            // (the stream's hardware queue is set up by its first launch: here, not in the build)
    (void)hipStreamSynchronize(c->stream);
    *out = c;
    return PQV_OK;
}
extern "C" int pqv_corpus_from_device(int device, const void *d_rows, uint64_t n, uint32_t dim,
                                      pqv_corpus **out) {
    return guard([&] { return pqv_corpus_from_device_impl(device, d_rows, n, dim, out); });
}

extern "C" uint64_t pqv_corpus_rows(const pqv_corpus *c) { return c ? c->n : 0; }
extern "C" uint32_t pqv_corpus_dim(const pqv_corpus *c) { return c ? c->dim : 0; }
extern "C" int pqv_corpus_device(const pqv_corpus *c) { return c ? c->device : -1; }

static int pqv_corpus_fetch_rows_impl(const pqv_corpus *c, const uint32_t *rows, uint64_t m,
                                     float *out) {
    if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
    if (m == 0) return PQV_OK;
    if (!rows || !out) return fail(PQV_ERR_INVALID, "rows/out must not be NULL");
    if (!c->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    for (uint64_t i = 0; i < m; ++i)
        if (rows[i] >= c->n) return fail(PQV_ERR_INVALID, "row id out of range");
    if (int rc = use_device(c->device)) return rc;
    DevBuf d_idx, d_out;
    HIP_TRY(d_idx.alloc(m * sizeof(uint32_t)));
    HIP_TRY(d_out.alloc(m * c->dim * sizeof(float)));
    HIP_TRY(hipMemcpy(d_idx.p, rows, m * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_TRY(pqv::launch_gather_rows(c->d_rows, d_idx.as<uint32_t>(), nullptr, m, c->dim,
                                    d_out.as<float>(), c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(hipMemcpy(out, d_out.p, m * c->dim * sizeof(float), hipMemcpyDeviceToHost));
    return PQV_OK;
}
extern "C" int pqv_corpus_fetch_rows(const pqv_corpus *c, const uint32_t *rows, uint64_t m,
                                     float *out) {
    return guard([&] { return pqv_corpus_fetch_rows_impl(c, rows, m, out); });
}

extern "C" void pqv_corpus_free(pqv_corpus *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

// ---------------------------------------------------------------------------------------
// index blob + accessors (src/ivf/index.rs:65-128)
// ---------------------------------------------------------------------------------------
namespace {
inline uint32_t rd_u32(const uint8_t *p) {
    return static_cast<uint32_t>(p[0]) | (static_cast<uint32_t>(p[1]) << 8) |
           (static_cast<uint32_t>(p[2]) << 16) | (static_cast<uint32_t>(p[3]) << 24);
}
inline void wr_u32(uint8_t *p, uint32_t v) {
    p[0] = static_cast<uint8_t>(v); p[1] = static_cast<uint8_t>(v >> 8);
    p[2] = static_cast<uint8_t>(v >> 16); p[3] = static_cast<uint8_t>(v >> 24);
}
}  // namespace

static int pqv_index_from_bytes_impl(const uint8_t *bytes, size_t len, pqv_index **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!bytes || len < 8) return fail(PQV_ERR_FORMAT, "IVF index buffer too small");  // index.rs:89
    const uint32_t dim = rd_u32(bytes), k = rd_u32(bytes + 4);
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");     // mod.rs:59
    if (k == 0) return fail(PQV_ERR_INVALID, "Cluster count must be > 0");             // index.rs:24
    size_t off = 8;
    const uint64_t clen = static_cast<uint64_t>(k) * dim;
    if ((len - off) / 4 < clen) return fail(PQV_ERR_FORMAT, "IVF index buffer truncated (centroids)");
    pqv_index *idx = new (std::nothrow) pqv_index();
    if (!idx) return fail(PQV_ERR_OOM, "host allocation failed");
    idx->dim = dim; idx->n_clusters = k;
    idx->centroids.resize(clen);
    for (uint64_t i = 0; i < clen; ++i, off += 4) {
        const uint32_t bits = rd_u32(bytes + off);
        std::memcpy(&idx->centroids[i], &bits, 4);
    }
    idx->list_off.assign(static_cast<size_t>(k) + 1, 0);
    size_t scan = off;
    for (uint32_t c = 0; c < k; ++c) {
        if (len - scan < 4) { delete idx; return fail(PQV_ERR_FORMAT, "IVF index buffer truncated (list length)"); }
        const uint32_t ll = rd_u32(bytes + scan);
        scan += 4;
        if ((len - scan) / 4 < ll) { delete idx; return fail(PQV_ERR_FORMAT, "IVF index buffer truncated (list rows)"); }
        scan += static_cast<size_t>(ll) * 4;
        idx->list_off[c + 1] = idx->list_off[c] + ll;
    }
    idx->list_rows.resize(idx->list_off[k]);
    for (uint32_t c = 0; c < k; ++c) {
        const uint32_t ll = rd_u32(bytes + off);
        off += 4;
        uint32_t *dst = idx->list_rows.data() + idx->list_off[c];
        for (uint32_t i = 0; i < ll; ++i, off += 4) dst[i] = rd_u32(bytes + off);
    }
    *out = idx;
    return PQV_OK;
}
extern "C" int pqv_index_from_bytes(const uint8_t *bytes, size_t len, pqv_index **out) {
    return guard([&] { return pqv_index_from_bytes_impl(bytes, len, out); });
}

static int pqv_index_to_bytes_impl(const pqv_index *idx, uint8_t **buf, size_t *len) {
    if (!idx || !buf || !len) return fail(PQV_ERR_INVALID, "index/buf/len must not be NULL");
    const uint64_t k = idx->n_clusters;
    const std::vector<uint32_t> *rows_p = idx->rows->get();
    if (!rows_p) return PQV_ERR_HIP;
    const std::vector<uint32_t> &rows_v = *rows_p;
    const size_t sz = 8 + idx->centroids.size() * 4 + static_cast<size_t>(k) * 4 + rows_v.size() * 4;
    uint8_t *b = static_cast<uint8_t *>(std::malloc(sz));
    if (!b) return fail(PQV_ERR_OOM, "host allocation failed");
    size_t off = 0;
    wr_u32(b, idx->dim); wr_u32(b + 4, idx->n_clusters); off = 8;
    for (float v : idx->centroids) {
        uint32_t bits;
        std::memcpy(&bits, &v, 4);
        wr_u32(b + off, bits);
        off += 4;
    }
    for (uint64_t c = 0; c < k; ++c) {
        const uint64_t s = idx->list_off[c], e = idx->list_off[c + 1];
        wr_u32(b + off, static_cast<uint32_t>(e - s));
        off += 4;
        for (uint64_t i = s; i < e; ++i, off += 4) wr_u32(b + off, rows_v[i]);
    }
    *buf = b;
    *len = sz;
    return PQV_OK;
}
extern "C" int pqv_index_to_bytes(const pqv_index *idx, uint8_t **buf, size_t *len) {
    return guard([&] { return pqv_index_to_bytes_impl(idx, buf, len); });
}

extern "C" void pqv_bytes_free(uint8_t *buf) { std::free(buf); }

static int pqv_index_from_parts_impl(uint32_t dim, uint32_t n_clusters, const float *centroids,
                                    const uint64_t *list_off, const uint32_t *list_rows,
                                    pqv_index **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");
    if (n_clusters == 0) return fail(PQV_ERR_INVALID, "Cluster count must be > 0");
    if (!centroids || !list_off) return fail(PQV_ERR_INVALID, "centroids/list_off must not be NULL");
    for (uint32_t c = 0; c < n_clusters; ++c)
        if (list_off[c + 1] < list_off[c]) return fail(PQV_ERR_INVALID, "list_off must be non-decreasing");
    if (list_off[0] != 0) return fail(PQV_ERR_INVALID, "list_off[0] must be 0");
    const uint64_t total = list_off[n_clusters];
    if (total && !list_rows) return fail(PQV_ERR_INVALID, "list_rows must not be NULL");
    pqv_index *idx = new (std::nothrow) pqv_index();
    if (!idx) return fail(PQV_ERR_OOM, "host allocation failed");
    idx->dim = dim; idx->n_clusters = n_clusters;
    idx->centroids.assign(centroids, centroids + static_cast<uint64_t>(n_clusters) * dim);
    idx->list_off.assign(list_off, list_off + n_clusters + 1);
    idx->list_rows.assign(list_rows, list_rows + total);
    *out = idx;
    return PQV_OK;
}
extern "C" int pqv_index_from_parts(uint32_t dim, uint32_t n_clusters, const float *centroids,
                                    const uint64_t *list_off, const uint32_t *list_rows,
                                    pqv_index **out) {
    return guard([&] { return pqv_index_from_parts_impl(dim, n_clusters, centroids, list_off, list_rows, out); });
}

extern "C" uint32_t pqv_index_dim(const pqv_index *i) { return i ? i->dim : 0; }
extern "C" uint32_t pqv_index_n_clusters(const pqv_index *i) { return i ? i->n_clusters : 0; }
extern "C" uint64_t pqv_index_n_rows(const pqv_index *i) { return i ? i->n_rows() : 0; }
extern "C" uint64_t pqv_index_row_bound(const pqv_index *i) {
    uint64_t b = 0;
    return i && i->row_bound(&b) ? b : 0;
}
extern "C" const float *pqv_index_centroids(const pqv_index *i) { return i ? i->centroids.data() : nullptr; }
extern "C" const uint64_t *pqv_index_list_offsets(const pqv_index *i) { return i ? i->list_off.data() : nullptr; }
extern "C" const uint32_t *pqv_index_list_rows(const pqv_index *i) {
    if (!i) return nullptr;
    const std::vector<uint32_t> *v = i->rows->get();         // (a build's lists are downloaded by the first reader)
    return v ? v->data() : nullptr;
}
extern "C" void pqv_index_free(pqv_index *i) { delete i; }

// ---------------------------------------------------------------------------------------
// k-means on the device (src/ivf/index.rs:323-457)
// ---------------------------------------------------------------------------------------
namespace {

// an on/off switch of the build: on unless the variable is set and starts with '0'
bool env_on(const char *name) { const char *e = std::getenv(name); return !(e && *e == '0'); }

// *nonfinite = some v[0 .. n) is inf / NaN: one flag round trip on the stream (flag: the caller's 4 bytes of device scratch)
int any_nonfinite(const float *v, uint64_t n, DevBuf &flag, hipStream_t stream, bool *nonfinite) {
    uint32_t h = 0;
    HIP_TRY(flag.ensure(sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), stream));
    HIP_TRY(pqv::launch_nonfinite_flag(v, n, flag.as<uint32_t>(), stream));
    HIP_TRY(hipMemcpyAsync(&h, flag.p, sizeof h, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *nonfinite = h != 0;
    return PQV_OK;
}

// Stable counting sort of rows by cluster == the reference's "ascending row ids per
// cluster" (index.rs:193-206).
// false if an assignment is out of range (a kernel bug must surface as an error, not as host memory corruption)
bool lists_from_assignment(const uint32_t *cluster_of, uint64_t n, uint32_t k,
                           std::vector<uint64_t> &off, std::vector<uint32_t> &rows) {
    // Large inputs: a stable counting sort over T contiguous row ranges on T host threads.  Range t's rows of a cluster
    // follow those of the ranges before it, so every list is in ascending row order -- the sequential scan's result.
    // PQV_LIST_THREADS=1 keeps the sequential scan (A/B)
    static const uint32_t t_max = [] { const char *e = std::getenv("PQV_LIST_THREADS"); const long v = e ? std::strtol(e, nullptr, 10) : 8;
                                       return static_cast<uint32_t>(std::min<long>(64, std::max<long>(1, v))); }();
    const uint32_t T = n >= (1u << 20) ? std::min<uint32_t>(t_max, std::max<uint32_t>(1, host_workers())) : 1;
    if (T > 1) {
        try {
            std::vector<uint64_t> cnt(static_cast<size_t>(T) * k, 0);
            std::atomic<bool> bad{false};
            auto run_ranges = [&](auto &&body) {
                std::vector<std::thread> th;
                th.reserve(T);
                for (uint32_t t = 0; t < T; ++t) th.emplace_back([&, t] { body(t, n * t / T, n * (t + 1) / T); });
                for (auto &x : th) x.join();
            };
            run_ranges([&](uint32_t t, uint64_t lo, uint64_t hi) {
                uint64_t *c = cnt.data() + static_cast<size_t>(t) * k;
                for (uint64_t r = lo; r < hi; ++r) {
                    const uint32_t v = cluster_of[r];
                    if (v >= k) { bad.store(true); return; }
                    c[v]++;
                }
            });
            if (bad.load()) return false;
            off.assign(static_cast<size_t>(k) + 1, 0);
            uint64_t run = 0;
            for (uint32_t c = 0; c < k; ++c) {
                off[c] = run;
                for (uint32_t t = 0; t < T; ++t) {
                    uint64_t &slot = cnt[static_cast<size_t>(t) * k + c];
                    const uint64_t x = slot;
                    slot = run;
                    run += x;
                }
            }
            off[k] = run;
            rows.resize(n);
            uint32_t *out = rows.data();
            run_ranges([&](uint32_t t, uint64_t lo, uint64_t hi) {
                uint64_t *cur = cnt.data() + static_cast<size_t>(t) * k;
                for (uint64_t r = lo; r < hi; ++r) out[cur[cluster_of[r]]++] = static_cast<uint32_t>(r);
            });
            return true;
        } catch (const std::system_error &) {
            // no threads to be had: the sequential scan below
        }
    }
    for (uint64_t r = 0; r < n; ++r) if (cluster_of[r] >= k) return false;
    off.assign(static_cast<size_t>(k) + 1, 0);
    for (uint64_t r = 0; r < n; ++r) off[cluster_of[r] + 1]++;
    for (uint32_t c = 0; c < k; ++c) off[c + 1] += off[c];
    rows.resize(n);
    std::vector<uint64_t> cur(off.begin(), off.end() - 1);
    for (uint64_t r = 0; r < n; ++r) rows[cur[cluster_of[r]]++] = static_cast<uint32_t>(r);
    return true;
}

// ---------------------------------------------------------------------------------------
// MFMA-screened assignment (index.rs:395-430 Lloyd assign, :189-206 + :244-257 final assignment).
// cluster[r] = argmin_j d2(x_r, c_j), strict '<' in ascending j, is the top-1 of row r among the
// centroids under the key (d2 bits, j) -- exactly what the wide screened search computes with the
// rows as queries and one list holding all centroids: thresholds from MFMA upper bounds of the first
// centroids (wide_seed_kernel), MFMA lower-bound screen of all of them, exact re-evaluation of the few
// survivors in the reference's summation order (wide_filter_kernel), top-1 merge.  The exact VALU
// kernel (assign_kernel) remains for dim % 64 != 0, for fewer than 512 centroids and for rows or
// centroids with a non-finite norm (NaN ordering is the reference's `<`, not the key order).
// ---------------------------------------------------------------------------------------
struct ScreenedAssign {
    static constexpr uint32_t width = 64;          // 64-row quads halve the re-streaming of the centroids
    static constexpr uint32_t rpb = 1024, seed_rows = 256;
    uint32_t dim = 0, kc = 0, chunk_q = 0, bpl = 0, max_quads = 0, ccap = 32;
    const float *d_centroids = nullptr;
    DevBuf cblk, cnorm, list_off, blk_off, flag;
    DevBuf qnorm, pairs, quads, nq_u32, cand_base, gthr, part_keys, part_vals, cand_keys, cand_vals, cand_cnt, spilled,
        seed_ub, qblk, dist_out, nfound;

    static bool applicable(uint32_t dim, uint32_t kc) {
        // PQV_ASSIGN_SCREEN=0 disables, =N (N > 1) sets the smallest centroid count that takes this path
        const char *e = std::getenv("PQV_ASSIGN_SCREEN");
        const long v = e ? std::strtol(e, nullptr, 10) : 512;
        return v != 0 && (dim % 64) == 0 && kc >= static_cast<uint32_t>(v > 1 ? v : 512);
    }
    // (re)load the centroids: blocked copy + norms; returns 1 in *nonfinite if a centroid norm is inf / NaN
    int set_centroids(const float *d_c, uint32_t k, uint32_t d, hipStream_t stream, bool *nonfinite) {
        using namespace pqv;
        dim = d; kc = k; d_centroids = d_c;
        chunk_q = 65536;          // (131072 / 262144 rows per chunk measured the same build time: the per-chunk launches are not what bounds it)
        bpl = (kc + rpb - 1) / rpb;
        max_quads = (chunk_q / width + 7) / 8 * 8;
        const uint64_t tiles = (static_cast<uint64_t>(kc) + 15) / 16;
        const uint64_t h_off[2] = {0, kc}, h_blk[2] = {0, tiles};
        HIP_TRY(list_off.ensure(sizeof h_off)); HIP_TRY(blk_off.ensure(sizeof h_blk)); HIP_TRY(flag.ensure(sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(list_off.p, h_off, sizeof h_off, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(blk_off.p, h_blk, sizeof h_blk, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));          // the two host arrays above are stack-allocated
        HIP_TRY(cblk.ensure(tiles * 16 * dim * sizeof(float)));
        HIP_TRY(cnorm.ensure(static_cast<size_t>(kc) * sizeof(float)));
        HIP_TRY(launch_row_norms(d_c, kc, dim, 1, cnorm.as<float>(), stream));
        if (int rc = any_nonfinite(cnorm.as<float>(), kc, flag, stream, nonfinite)) return rc;
        HIP_TRY(launch_block_rows(d_c, list_off.as<uint64_t>(), blk_off.as<uint64_t>(), 1, tiles, dim, cblk.p, stream));
        return PQV_OK;
    }
    // cluster[0 .. n) for rows d_rows[0 .. n); *fallback = true if a row norm is not finite (nothing written)
    int run(const float *d_rows, uint64_t n, uint32_t *d_cluster, hipStream_t stream, bool *fallback) {
        using namespace pqv;
        *fallback = false;
        HIP_TRY(qnorm.ensure(static_cast<size_t>(n) * sizeof(float)));
        HIP_TRY(launch_row_norms(d_rows, n, dim, 1, qnorm.as<float>(), stream));
        bool bad = false;
        if (int rc = any_nonfinite(qnorm.as<float>(), n, flag, stream, &bad)) return rc;
        if (bad) { *fallback = true; return PQV_OK; }
        const uint32_t k = 1, slots = 4 * bpl, seed_sw = 4;
        HIP_TRY(pairs.ensure(static_cast<size_t>(chunk_q) * 4)); HIP_TRY(quads.ensure(static_cast<size_t>(max_quads) * sizeof(uint4)));
        HIP_TRY(nq_u32.ensure(16)); HIP_TRY(cand_base.ensure(static_cast<size_t>(chunk_q) * 8));
        HIP_TRY(gthr.ensure(static_cast<size_t>(chunk_q) * 8));
        const uint64_t entries = (static_cast<uint64_t>(chunk_q) * slots * k + 3) / 4 * 4;
        HIP_TRY(part_keys.ensure((entries + 4) * 8)); HIP_TRY(part_vals.ensure((entries + 4) * 4));
        HIP_TRY(cand_keys.ensure(static_cast<size_t>(chunk_q) * ccap * 8)); HIP_TRY(cand_vals.ensure(static_cast<size_t>(chunk_q) * ccap * 4));
        HIP_TRY(cand_cnt.ensure(static_cast<size_t>(chunk_q) * 4)); HIP_TRY(spilled.ensure(static_cast<size_t>(chunk_q) * 4));
        HIP_TRY(seed_ub.ensure(static_cast<size_t>(chunk_q) * seed_sw * 16 * 4));
        HIP_TRY(dist_out.ensure(static_cast<size_t>(chunk_q) * 4)); HIP_TRY(nfound.ensure(static_cast<size_t>(chunk_q) * 4));
        const bool qlds = static_cast<uint64_t>(width) * dim * sizeof(float) <= 32768;
        if (!qlds) HIP_TRY(qblk.ensure(static_cast<size_t>(max_quads) * width * dim * sizeof(float)));
        for (uint64_t r0 = 0; r0 < n; r0 += chunk_q) {
            const uint32_t nq = static_cast<uint32_t>(std::min<uint64_t>(chunk_q, n - r0));
            const float *q = d_rows + r0 * dim;
            HIP_TRY(launch_assign_setup(pairs.as<uint32_t>(), quads.as<uint4>(), nq_u32.as<uint32_t>(), cand_base.as<uint64_t>(),
                                        gthr.as<unsigned long long>(), nq, width, stream));
            HIP_TRY(launch_fill_ones2(part_keys.p, entries * 8, part_vals.p, entries * 4, stream));
            TileArgs ta{};
            ta.mat = d_centroids; ta.row_of = nullptr; ta.list_off = list_off.as<uint64_t>();
            ta.queries = q; ta.cand_base = cand_base.as<uint64_t>(); ta.pairs = pairs.as<uint32_t>();
            ta.quads = quads.as<uint4>(); ta.n_quads = nq_u32.as<uint32_t>(); ta.max_quads = max_quads; ta.quad_width = width;
            ta.max_groups = max_quads;          // only its being non-zero matters to the launcher
            ta.nq = nq; ta.nprobe = 1; ta.dim = dim; ta.k = k;
            ta.rows_per_block = rpb; ta.blocks_per_list = bpl; ta.max_pos = ~0ull;
            ta.slots_per_pair = slots; ta.slot_base = 0; ta.n_part = slots;
            ta.gthr = gthr.as<unsigned long long>();
            ta.part_keys = part_keys.as<uint64_t>(); ta.part_vals = part_vals.as<uint32_t>();
            ta.mat_blk = static_cast<const float4 *>(cblk.p); ta.blk_off = blk_off.as<uint64_t>();
            ta.row_norm2 = cnorm.as<float>(); ta.query_norm2 = qnorm.as<float>() + r0;
            ta.cand_keys = cand_keys.as<uint64_t>(); ta.cand_vals = cand_vals.as<uint32_t>();
            ta.cand_cnt = cand_cnt.as<uint32_t>(); ta.cand_cap = ccap; ta.spilled = spilled.as<uint32_t>();
            ta.xcd_swizzle = qlds ? 0 : 1;
            if (!qlds) {
                HIP_TRY(launch_pack_queries(q, ta.pairs, ta.quads, ta.n_quads, max_quads, 1, dim, width / 16, qblk.p, stream));
                ta.q_blk = static_cast<const float4 *>(qblk.p);
            }
            TileArgs seed = ta;
            seed.row_offset = 0; seed.row_end = seed_rows; seed.rows_per_block = 256; seed.grid_x = 1;
            seed.seed_sw = seed_sw; seed.seed_ub = seed_ub.as<float>();
            HIP_TRY(launch_wide_seed(seed, stream));
            HIP_TRY(launch_seed_select(seed.seed_ub, nq, seed_sw * 16, k, ta.gthr, ta.cand_cnt, ta.spilled, stream));
            ta.row_offset = 0; ta.grid_x = bpl; ta.filter_variant = 0;
            HIP_TRY(launch_tile_filter(ta, stream));
            MergeArgs fm{};
            fm.part_keys = ta.part_keys; fm.part_vals = ta.part_vals;
            fm.nq = nq; fm.n_part = slots; fm.k_part = k; fm.k = k; fm.k_out = k;
            fm.ids = nullptr; fm.row_idx = d_cluster + r0; fm.dist = dist_out.as<float>(); fm.n_found = nfound.as<uint32_t>();
            fm.sqrt_out = 0;
            fm.cand_keys = ta.cand_keys; fm.cand_vals = ta.cand_vals; fm.cand_cnt = ta.cand_cnt; fm.cand_cap = ccap;
            fm.spilled = ta.spilled;
            HIP_TRY(launch_merge_final(fm, stream));
        }
        return PQV_OK;
    }
};

// ---------------------------------------------------------------------------------------
// Round 3: the assignment as a dense f16 contraction + exact re-scoring (kernels_build.hip: assign_f16_kernel,
// assign_rescore_kernel).  Rows and centroids are imaged as unit vectors about a common centre mu (the column mean of
// the centroids: the distance is translation invariant, and |x - mu| |c - mu| is what scales the bound's slack); the
// screen leaves a handful of candidate centroids per row, the exact pass evaluates those in the reference's order and
// takes the argmin by (distance bits, index) -- index.rs:408-415's strict '<' in ascending order.  Needs dim % 4 == 0
// and finite norms (NaN ordering is the reference's `<`, not the key order): otherwise the callers keep their old path.
// ---------------------------------------------------------------------------------------
struct GemmAssign {
    uint32_t dim = 0, dim_p = 0, kc = 0, kc_pad = 0, cap = 32;
    uint64_t chunk = [] { const char *e = std::getenv("PQV_ASSIGN_CHUNK"); const long v = e ? std::atol(e) : 0; return v >= 4096 ? static_cast<uint64_t>(v) : (1ull << 18); }();
    const float *d_centroids = nullptr;
    DevBuf mu, c16, cn2, x16, xn2, cand, cnt, flag, cand_t, best_t, rstats, d_perm, d_grp;
    // round 4: 256 x 256 tiles with the rows on the lane-owned side and centroid images at one global scale (assign_wide_kernel +
    // assign_resolve_kernel); PQV_ASSIGN_TILE=128 keeps round 3's 128 x 256 kernel with its own exact pass (A/B, tests)
    bool wide = true;
    // The Lloyd iterations assign the SAME rows again and again: with the centring vector kept from the first iteration (any fixed
    // vector serves the bounds; the first centroid mean is as good as the current one) the rows' images and norms are made once.
    std::vector<uint32_t> h_perm; std::vector<float> h_grp;
    bool keep_mu = false, mu_set = false;
    const float *img_rows = nullptr; uint64_t img_n = 0; uint32_t img_dim_p = 0;       // what x16 / xn2 currently hold (single-chunk runs)
    float cmaxs = 0.0f, cn_max = 0.0f, kA = 0.0f;
    std::vector<float> h_cn2;
    unsigned long long exact_rows = 0, exact_evals = 0, rows_total = 0;

    static bool applicable(uint32_t dim, uint32_t kc) {
        const char *e = std::getenv("PQV_ASSIGN_GEMM");          // 0 = off, n > 1 = smallest centroid count that takes this path
        const long v = e ? std::strtol(e, nullptr, 10) : 128L;
        return v != 0 && (dim % 4) == 0 && kc >= static_cast<uint32_t>(v > 1 ? v : 128) && static_cast<uint64_t>((dim + 31) / 32 * 32) * 2 * 320 < 0x7FFFFFFFull;
    }
    int set_centroids(const float *d_c, uint32_t k, uint32_t d, hipStream_t stream, bool *nonfinite) {
        using namespace pqv;
        {
            const char *e = std::getenv("PQV_ASSIGN_TILE");
            wide = !(e && std::atoi(e) == 128) && static_cast<uint64_t>((d + 63) / 64 * 64) * 2 * 512 < 0x7FFFFFFFull;
        }
        dim = d; dim_p = wide ? (d + 63) / 64 * 64 : (d + 31) / 32 * 32; kc = k; kc_pad = (k + 255) / 256 * 256; d_centroids = d_c;
        HIP_TRY(mu.ensure(static_cast<size_t>(dim) * sizeof(float)));
        HIP_TRY(c16.ensure(static_cast<size_t>(kc_pad) * dim_p * sizeof(uint16_t)));
        HIP_TRY(cn2.ensure(static_cast<size_t>(kc_pad) * sizeof(float)));
        if (!(keep_mu && mu_set)) { HIP_TRY(launch_col_mean(d_c, kc, dim, mu.as<float>(), stream)); mu_set = true; img_rows = nullptr; }
        HIP_TRY(launch_center_normalize_f16(d_c, mu.as<float>(), kc, kc_pad, dim, dim_p, cn2.as<float>(), c16.p, stream));
        if (!wide) return any_nonfinite(cn2.as<float>(), kc, flag, stream, nonfinite);
        // one global scale for the centroid images: 2^8 / max |c - mu| (the norms come back anyway: this is the call's one host check)
        h_cn2.resize(kc);
        HIP_TRY(hipMemcpyAsync(h_cn2.data(), cn2.p, static_cast<size_t>(kc) * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        float mx = 0.0f;
        bool bad = false;
        for (float v : h_cn2) { if (!(v <= 3.0e38f)) bad = true; else mx = std::max(mx, v); }
        *nonfinite = bad;
        if (bad) return PQV_OK;
        cn_max = mx * 1.000001f;
        cmaxs = std::sqrt(mx) * 1.000001f;
        const float cscale = cmaxs > 0.0f ? 256.0f / cmaxs : 0.0f;
        if (!(cscale > 0.0f && cscale < 3.0e38f)) { wide = false; return PQV_OK; }      // all centroids at mu / degenerate scale: round 3's kernel (images already written)
        kA = 2.0f / (256.0f * cscale);
        // images in ascending-norm order: a 32-centroid group's own largest norm scales its error bound (a table trained on a
        // sample has a few far-out centroids -- clusters of one or two points -- and the table-wide maximum would loosen every bound)
        std::vector<uint32_t> &perm = h_perm;          // (members: the uploads below need no synchronisation to outlive)
        std::vector<float> &grp = h_grp;
        perm.resize(kc);
        for (uint32_t c = 0; c < kc; ++c) perm[c] = c;
        std::stable_sort(perm.begin(), perm.end(), [&](uint32_t x, uint32_t y) { return h_cn2[x] < h_cn2[y]; });
        const uint32_t ngrp = kc_pad / 32;
        grp.assign(2 * static_cast<size_t>(ngrp), 0.0f);
        for (uint32_t g = 0; g < ngrp; ++g) {
            float gm = 0.0f;
            for (uint32_t s = g * 32; s < std::min(kc, (g + 1) * 32); ++s) gm = std::max(gm, h_cn2[perm[s]]);
            grp[g] = std::sqrt(gm) * 1.000001f; grp[ngrp + g] = gm * 1.000001f;
        }
        HIP_TRY(d_perm.ensure(static_cast<size_t>(kc) * sizeof(uint32_t)));
        HIP_TRY(d_grp.ensure(grp.size() * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(d_perm.p, perm.data(), static_cast<size_t>(kc) * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(d_grp.p, grp.data(), grp.size() * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(launch_center_normalize_f16(d_c, mu.as<float>(), kc, kc_pad, dim, dim_p, cn2.as<float>(), c16.p, stream, cscale, d_perm.as<uint32_t>()));
        return PQV_OK;          // (perm / grp are members: a later call rewrites them only after its own synchronisation on the norms)
    }
    // cluster[0 .. n) for rows d_rows[0 .. n); *fallback = true if a row norm is not finite (the caller re-runs its old path)
    // (Measured and dropped: the assignment copied to the host chunk by chunk on a second stream behind the next chunk's kernels -- a
    //  device-to-pageable copy there stalls the compute stream's queue, 53 ms for the loop against 34 ms of kernels on C3.)
    int run(const float *d_rows, uint64_t n, uint32_t *d_cluster, hipStream_t stream, bool *fallback) {
        using namespace pqv;
        *fallback = false;
        const double t_run0 = now_s();
        const uint64_t ch = std::min<uint64_t>(chunk, std::max<uint64_t>(1, n));
        HIP_TRY(x16.ensure(ch * dim_p * sizeof(uint16_t)));
        HIP_TRY(xn2.ensure(ch * sizeof(float)));
        HIP_TRY(cand.ensure(ch * cap * sizeof(uint32_t)));
        HIP_TRY(cnt.ensure(ch * sizeof(uint32_t)));
        if (wide) {
            HIP_TRY(cand_t.ensure(ch * cap * sizeof(float)));
            HIP_TRY(best_t.ensure(ch * sizeof(float)));
            HIP_TRY(rstats.ensure(2 * sizeof(unsigned long long)));
            HIP_TRY(hipMemsetAsync(rstats.p, 0, 2 * sizeof(unsigned long long), stream));
        }
        const float eps = 1.01f * 9.765625e-04f + 2.0f * static_cast<float>(dim_p) * 5.9604645e-08f + 2.0e-6f;
        const float cm = static_cast<float>(dim + 16) * 2.384185791015625e-07f;
        // (one host check of the row norms after all chunks: a non-finite one sends the whole call to the caller's old path)
        HIP_TRY(flag.ensure(sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(flag.p, 0, sizeof(uint32_t), stream));
        for (uint64_t r0 = 0; r0 < n; r0 += ch) {
            const uint64_t m = std::min<uint64_t>(ch, n - r0);
            const float *rows = d_rows + r0 * dim;
            const bool have_img = keep_mu && n <= ch && img_rows == d_rows && img_n == n && img_dim_p == dim_p;
            if (!have_img) HIP_TRY(launch_center_normalize_f16(rows, mu.as<float>(), m, m, dim, dim_p, xn2.as<float>(), x16.p, stream));
            HIP_TRY(launch_nonfinite_flag(xn2.as<float>(), m, flag.as<uint32_t>(), stream));
            img_rows = n <= ch ? d_rows : nullptr; img_n = n; img_dim_p = dim_p;
            HIP_TRY(hipMemsetAsync(cnt.p, 0, m * sizeof(uint32_t), stream));
            if (wide) {
                AssignWideArgs w{};
                w.x16 = x16.as<uint16_t>(); w.c16 = c16.as<uint16_t>(); w.xn2 = xn2.as<float>(); w.cn2 = cn2.as<float>();
                w.perm = d_perm.as<uint32_t>(); w.grp_cs = d_grp.as<float>(); w.grp_cn = d_grp.as<float>() + kc_pad / 32;
                w.m = m; w.kc = kc; w.kc_pad = kc_pad; w.dim_p = dim_p; w.kA = kA; w.eps = eps;
                // the reference's summation margin, tight: a squared difference carries <= 3 roundings, the 4-group <= 3 more, the
                // running sum one per group (index.rs:461-480; all terms non-negative) -- (dim / 4 + 6) 2^-24, taken twice over
                w.cm = static_cast<float>(dim / 4 + 16) * 1.1920928955078125e-07f;
                w.cand = cand.as<uint32_t>(); w.cand_t = cand_t.as<float>(); w.cand_cnt = cnt.as<uint32_t>(); w.best_t = best_t.as<float>(); w.cap = cap;
                // (the final assignment brackets the contraction kernel with HIP events -- time_kernels: the roofline of bench.py's
                //  index_build record divides by KERNEL time, not by the phase's wall time)
                hipEvent_t e0 = nullptr, e1 = nullptr;
                if (time_kernels) {
                    HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1));
                    kernel_ev.push_back(e0); kernel_ev.push_back(e1);
                    HIP_TRY(hipEventRecord(e0, stream));
                }
                HIP_TRY(launch_assign_wide(w, stream));
                if (time_kernels) HIP_TRY(hipEventRecord(e1, stream));
                // (the two counters are same-address atomics from every wave: diagnostic runs only)
                HIP_TRY(launch_assign_resolve(w, rows, d_centroids, dim, d_cluster + r0, verbose() ? rstats.as<unsigned long long>() : nullptr, stream));
            } else {
            AssignF16Args a{};
            a.x16 = x16.as<uint16_t>(); a.c16 = c16.as<uint16_t>(); a.xn2 = xn2.as<float>(); a.cn2 = cn2.as<float>();
            a.m = m; a.kc = kc; a.kc_pad = kc_pad; a.dim_p = dim_p; a.eps = eps; a.cm = cm;
            a.cand = cand.as<uint32_t>(); a.cand_cnt = cnt.as<uint32_t>(); a.cap = cap;
            HIP_TRY(launch_assign_f16(a, stream));
            HIP_TRY(launch_assign_rescore(rows, d_centroids, m, dim, kc, cand.as<uint32_t>(), cnt.as<uint32_t>(), cap, d_cluster + r0, stream));
            }
            if (verbose() && r0 == 0 && n >= 65536) {      // candidates the screen left per row (first chunk)
                std::vector<uint32_t> hc(m);
                HIP_TRY(hipMemcpyAsync(hc.data(), cnt.p, m * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
                HIP_TRY(hipStreamSynchronize(stream));
                uint64_t sum = 0, over = 0; uint32_t mx = 0;
                for (uint32_t c : hc) { sum += c; mx = std::max(mx, c); over += c > cap; }
                std::fprintf(stderr, "[pqv] f16 assignment: %.2f candidates per row (max %u, %llu rows over the %u-entry list) of %u centroids\n",
                             static_cast<double>(sum) / static_cast<double>(m), mx, (unsigned long long)over, cap, kc);
            }
        }
        const double t_run1 = now_s();
        uint32_t h = 0;
        HIP_TRY(hipMemcpyAsync(&h, flag.p, sizeof h, hipMemcpyDeviceToHost, stream));
        if (verbose() && n >= (1u << 20)) std::fprintf(stderr, "[pqv] f16 assignment: %llu rows enqueued in %.1f ms\n", (unsigned long long)n,
                                                       (t_run1 - t_run0) * 1e3);
        if (wide && verbose()) {
            unsigned long long hs[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(hs, rstats.p, sizeof hs, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            exact_rows += hs[0]; exact_evals += hs[1]; rows_total += n;
            if (n >= 65536) std::fprintf(stderr, "[pqv] f16 assignment (256 x 256 tiles): %.1f %% of %llu rows evaluated exactly, %.2f evaluations per such row\n",
                                         100.0 * static_cast<double>(hs[0]) / static_cast<double>(n), (unsigned long long)n,
                                         hs[0] ? static_cast<double>(hs[1]) / static_cast<double>(hs[0]) : 0.0);
        }
        HIP_TRY(hipStreamSynchronize(stream));
        if (!kernel_ev.empty()) {
            double ms_sum = 0.0;
            for (size_t i = 0; i + 1 < kernel_ev.size(); i += 2) {
                float ms = 0.0f;
                if (hipEventElapsedTime(&ms, kernel_ev[i], kernel_ev[i + 1]) == hipSuccess) ms_sum += ms;
            }
            g_build_stats[BS_WIDE_KERNEL_S] = ms_sum * 1e-3; g_build_stats[BS_WIDE_LAUNCHES] = static_cast<double>(kernel_ev.size() / 2);
            for (hipEvent_t e : kernel_ev) (void)hipEventDestroy(e);
            kernel_ev.clear();
        }
        *fallback = h != 0;
        return PQV_OK;
    }
    std::vector<hipEvent_t> kernel_ev;
    bool time_kernels = false;
    // (an early error return of run() leaves its events here)
    ~GemmAssign() { for (hipEvent_t e : kernel_ev) (void)hipEventDestroy(e); }
};

// acc[c] = ((0 + m[0][c]) + m[1][c]) + ... + m[rows - 1][c] for c in [0, width), width a multiple of 16: `width` independent f32
// chains, each in its own sequential order (element-wise vector adds do not re-associate anything).  The AVX2 body is chosen at
// run time; both bodies add the same operands in the same order, so the sums are identical bit for bit.
typedef float v4f_t __attribute__((vector_size(16), aligned(4)));
typedef float v8f_t __attribute__((vector_size(32), aligned(4)));
// k-means++ pick (index.rs:372-383): the first slot whose SEQUENTIAL f32 cumulative sum reaches `gen_range(0.0..1.0) * total`.  The
// cumulative sum does not depend on the threshold, and `total` (the chunk sums of :356-370, ~6 us per round) does not depend on the
// cumulative sum: a second host thread starts the walk the moment a round's minima are final, keeping the prefix it has passed; when
// the main thread publishes the threshold it looks back through that prefix (linearly: the reference's "first slot", whatever the
// values -- a NaN makes the prefix non-monotone) or walks on with the reference's own compare.  The same adds in the same order on
// the same values: the pick is the reference's.
struct PrefixScout {
    const float *md = nullptr;
    uint64_t n = 0;
    std::vector<float> prefix;
    alignas(64) std::atomic<uint32_t> req{0};          // main -> scout: walk round r (0: none yet; ~0u: exit)
    alignas(64) std::atomic<uint32_t> thr_round{0};    // main -> scout: round whose threshold (or cancellation) is published
    float thr_value = 0.0f;
    bool cancel = false;
    alignas(64) std::atomic<uint32_t> res_round{0};    // scout -> main: round whose result is published
    uint64_t res_slot = ~0ull;
    std::thread th;
    static void relax() {
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
    void run() {
        uint32_t seen = 0;
        for (;;) {
            uint32_t r;
            while ((r = req.load(std::memory_order_acquire)) == seen) relax();
            if (r == ~0u) return;
            seen = r;
            float cumsum = 0.0f;
            uint64_t pos = 0, found = ~0ull;
            bool have_thr = false, stop = false;
            float thr = 0.0f;
            while (!have_thr && pos < n) {                     // the threshold is not known yet: walk and remember
                const uint64_t e = pos + 64 < n ? pos + 64 : n;
                for (; pos < e; ++pos) { cumsum = cumsum + md[pos]; prefix[pos] = cumsum; }
                if (thr_round.load(std::memory_order_acquire) == r) have_thr = true;
                else if (req.load(std::memory_order_acquire) == ~0u) return;          // (the build failed half-way through a round)
            }
            while (!have_thr) {                                // (walked to the end before the total was there)
                if (thr_round.load(std::memory_order_acquire) == r) have_thr = true;
                else if (req.load(std::memory_order_acquire) == ~0u) return;
                else relax();
            }
            thr = thr_value; stop = cancel;
            if (!stop) {
                for (uint64_t i = 0; i < pos; ++i)             // what has been passed already: the FIRST slot at or above the threshold
                    if (prefix[i] >= thr) { found = i; break; }
                if (found == ~0ull)
                    for (; pos < n; ++pos) {                   // index.rs:375-383 from here on
                        cumsum = cumsum + md[pos];
                        if (cumsum >= thr) { found = pos; break; }
                    }
            }
            res_slot = found;
            res_round.store(r, std::memory_order_release);
        }
    }
    void start(const float *minima, uint64_t count) {
        md = minima; n = count; prefix.assign(count, 0.0f);
        th = std::thread([this] { run(); });
    }
    void begin(uint32_t r) { req.store(r, std::memory_order_release); }
    uint64_t finish(uint32_t r, float threshold, bool cancelled) {
        thr_value = threshold; cancel = cancelled;
        thr_round.store(r, std::memory_order_release);
        while (res_round.load(std::memory_order_acquire) != r) relax();
        return res_slot;
    }
    ~PrefixScout() {
        if (th.joinable()) { req.store(~0u, std::memory_order_release); th.join(); }
    }
};

__attribute__((target("avx2"))) static void chain_sums_avx2(const float *m, uint64_t rows, uint64_t width, float *acc) {
    for (uint64_t c0 = 0; c0 < width; c0 += 32) {          // four 8-lane accumulators: 32 chains per pass over the rows
        const uint64_t nb = std::min<uint64_t>(4, (width - c0) / 8);
        v8f_t s[4] = {{0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}, {0, 0, 0, 0, 0, 0, 0, 0}};
        for (uint64_t t = 0; t < rows; ++t) {
            const float *r = m + t * width + c0;
            for (uint64_t b = 0; b < nb; ++b) s[b] = s[b] + *reinterpret_cast<const v8f_t *>(r + 8 * b);
        }
        for (uint64_t b = 0; b < nb; ++b) *reinterpret_cast<v8f_t *>(acc + c0 + 8 * b) = s[b];
    }
}
static void chain_sums(const float *m, uint64_t rows, uint64_t width, float *acc) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2) { chain_sums_avx2(m, rows, width, acc); return; }
    for (uint64_t c0 = 0; c0 < width; c0 += 16) {
        v4f_t s[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
        for (uint64_t t = 0; t < rows; ++t) {
            const float *r = m + t * width + c0;
            for (int b = 0; b < 4; ++b) s[b] = s[b] + *reinterpret_cast<const v4f_t *>(r + 4 * b);
        }
        for (int b = 0; b < 4; ++b) *reinterpret_cast<v4f_t *>(acc + c0 + 4 * b) = s[b];
    }
}

// The inverted lists built on the device (kernels_build.hip: launch_list_sort) -- the same ascending-row-id lists as
// lists_from_assignment above, without the assignment's trip to the host.  PQV_DEVICE_LISTS=0 keeps the host sort (A/B).
struct DeviceLists {
    DevBuf cnt, tot, bad;
    uint32_t rpb = 4096;
    static bool applicable(uint64_t n, uint32_t k) {
        static const bool on = env_on("PQV_DEVICE_LISTS");
        return on && n > 0 && n <= 0xFFFFFFFFull && k > 0 && k <= 4096;
    }
    int prepare(uint64_t n, uint32_t k) {
        // blocks of 4096 rows; below 2^20 rows smaller blocks keep a few hundred of them in flight
        rpb = n >= (1u << 20) ? 4096 : n >= (1u << 17) ? 1024 : 256;
        const uint64_t nblk = (n + rpb - 1) / rpb;
        HIP_TRY(cnt.alloc(static_cast<size_t>(k) * nblk * sizeof(uint32_t)));
        HIP_TRY(tot.alloc(static_cast<size_t>(k) * sizeof(unsigned long long)));
        HIP_TRY(bad.alloc(sizeof(uint32_t)));
        return PQV_OK;
    }
    // enqueues the sort; *bad stays 0 unless an assignment is out of range (check() after the stream drained)
    int run(const uint32_t *d_assign, uint64_t n, uint32_t k, uint64_t *d_list_off, uint32_t *d_list_rows, hipStream_t stream) {
        HIP_TRY(hipMemsetAsync(bad.p, 0, sizeof(uint32_t), stream));
        HIP_TRY(pqv::launch_list_sort(d_assign, n, k, cnt.as<uint32_t>(), rpb, tot.as<unsigned long long>(), d_list_off, d_list_rows,
                                 bad.as<uint32_t>(), stream));
        return PQV_OK;
    }
};

// The assignment ladder (index.rs:395-430 in Lloyd; :189-206 + :244-257 in assign_rows): cluster[r] = the nearest centroid of row r
// by the f16 contraction (GemmAssign), else by the f32 MFMA screen (ScreenedAssign), else by the exact kernel.  A tier steps down
// where a centroid norm (its set_centroids) or a row norm (its run) is not finite: NaN ordering is the reference's `<`, which only
// the exact kernel keeps.  The caller chooses the tiers to try once; Lloyd keeps one ladder over its iterations, so the
// contraction's centring vector and row images carry over (GemmAssign::keep_mu).
struct AssignLadder {
    enum Tier { EXACT = 0, SCREEN = 1, GEMM = 2 };         // (the values of BS_FINAL_FORM / BS_LLOYD_FORM)
    GemmAssign gemm;
    ScreenedAssign screen;
    bool try_gemm = false, try_screen = false;
    // one call on a local ladder (assign_rows): the stream is drained behind each tier, before the next one starts and before the
    // scope exit releases the tiers' buffers; t0 is the clock origin of that call's PQV_VERBOSE lines
    bool one_shot = false;
    double t0 = 0.0;
    // d_cluster[i] = nearest centroid of row i of d_rows [n, dim], i in [0, n); *decided = the tier that wrote it.  With d_prev and
    // d_changed (Lloyd, :417-427) *d_changed counts the rows whose cluster differs from d_prev's: the exact kernel counts as it
    // assigns, a tier above it is followed by count_changed_kernel.
    int run(const float *d_rows, uint64_t n, const float *d_centroids, uint32_t k, uint32_t dim, uint32_t *d_cluster, hipStream_t stream,
            Tier *decided, const uint32_t *d_prev = nullptr, unsigned long long *d_changed = nullptr) {
        using namespace pqv;
        *decided = EXACT;
        auto attempt = [&](auto &tier, Tier t, bool trace) -> int {
            bool bad_c = false, bad_r = false;
            if (int rc = tier.set_centroids(d_centroids, k, dim, stream, &bad_c)) return rc;
            if (trace) std::fprintf(stderr, "[pqv] final assignment: centroids set at %.1f ms\n", (now_s() - t0) * 1e3);
            if (!bad_c) { if (int rc = tier.run(d_rows, n, d_cluster, stream, &bad_r)) return rc; }
            if (one_shot) HIP_TRY(hipStreamSynchronize(stream));
            if (trace) std::fprintf(stderr, "[pqv] final assignment: f16 path done at %.1f ms\n", (now_s() - t0) * 1e3);
            if (!bad_c && !bad_r) *decided = t;
            return PQV_OK;
        };
        if (try_gemm) { if (int rc = attempt(gemm, GEMM, one_shot && verbose())) return rc; }
        if (*decided == EXACT && try_screen) { if (int rc = attempt(screen, SCREEN, false)) return rc; }
        if (*decided == EXACT) HIP_TRY(launch_assign(d_rows, n, dim, d_centroids, k, d_cluster, d_prev, d_changed, nullptr, stream));
        else if (d_changed) HIP_TRY(launch_count_changed(d_cluster, d_prev, n, d_changed, stream));
        return PQV_OK;
    }
};

// k-means++ (index.rs:332-390) in stages, each owning its buffers; kmeans_device below strings them together.

// The subset the rounds run over (:332-338): every row up to 50 000 of them, else an index_sample gathered into a buffer of its own.
struct KppSubset {
    uint64_t init_n = 0;
    uint32_t dim = 0;
    const float *d_init = nullptr;
    std::vector<uint64_t> indices;
    DevBuf d_own, d_idx;
    int draw(pqv::StdRng &rng, const float *d_data, uint64_t n, uint32_t row_dim, uint32_t k, hipStream_t stream) {
        init_n = std::max<uint64_t>(std::min<uint64_t>(n, 50000), k); dim = row_dim; d_init = d_data;
        if (init_n == n) return PQV_OK;
        indices = index_sample(rng, n, init_n);
        HIP_TRY(d_idx.alloc(init_n * sizeof(uint64_t)));
        HIP_TRY(d_own.alloc(init_n * dim * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(d_idx.p, indices.data(), init_n * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(pqv::launch_gather_rows(d_data, nullptr, d_idx.as<uint64_t>(), init_n, dim, d_own.as<float>(), stream));
        d_init = d_own.as<float>();
        return PQV_OK;
    }
    const float *row(uint64_t pick) const { return d_init + pick * dim; }
    void release() { d_own.release(); d_idx.release(); }
};

// min_distances (:344-352): the minima on the device, mirrored by the update kernels into pinned host memory where the host sums
// and walks them, and the worker chunking of their sum (:259-265, :305-306).
// With many chunks (a 256-core host: 256 chunks of 196 minima) the independent chunk chains are added as vector lanes: the kernels
// keep a second mirror in chunk-transposed order [position in chunk][chunk] (padding stays +0.0: x + 0.0 == x for the non-negative
// sums), and step t adds row t of it to the running sums -- every chain still in its own order.
struct KppMinima {
    uint64_t n = 0, chunk = 0, n_chunks = 0, wpad = 0;
    bool use_t = false;
    uint32_t mirror_chunk = 0, mirror_stride = 0;      // what the kernels' arguments of those names take (0 without the transposed mirror)
    DevBuf d_min;
    PinnedBuf h_min, h_min_t;
    std::vector<float> chain_acc;

    int init(uint64_t init_n, uint32_t workers, hipStream_t stream) {
        n = init_n;
        const uint64_t w = std::max<uint64_t>(1, std::min<uint64_t>(workers, n));
        chunk = (n + w - 1) / w;
        n_chunks = (n + chunk - 1) / chunk;
        wpad = (n_chunks + 15) / 16 * 16;
        use_t = n_chunks >= 16 && chunk * wpad <= (64ull << 20);
        HIP_TRY(d_min.alloc(n * sizeof(float)));
        std::vector<float> inf(n, INFINITY);
        HIP_TRY(hipMemcpyAsync(d_min.p, inf.data(), n * sizeof(float), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        HIP_TRY(h_min.ensure(n * sizeof(float)));
        if (use_t) {
            HIP_TRY(h_min_t.ensure(chunk * wpad * sizeof(float)));
            float *mt = h_min_t.as<float>();
            for (uint64_t t = 0; t < chunk * wpad; ++t) mt[t] = 0.0f;
            mirror_chunk = static_cast<uint32_t>(chunk); mirror_stride = static_cast<uint32_t>(wpad);
            chain_acc.resize(wpad);
        }
        fill_mirrors(inf.data());                      // the mirrors start equal to d_min
        return PQV_OK;
    }
    float *mirror() const { return h_min.as<float>(); }
    float *mirror_t() const { return use_t ? h_min_t.as<float>() : nullptr; }
    // both mirrors from the minima in slot order (md may be the plain mirror itself)
    void fill_mirrors(const float *md) {
        if (md != mirror()) std::memcpy(mirror(), md, n * sizeof(float));
        if (!use_t) return;
        float *mt = h_min_t.as<float>();
        for (uint64_t pos = 0; pos < n; ++pos) mt[(pos % chunk) * wpad + pos / chunk] = md[pos];
    }
    // the mirrors as the device holds the minima now (behind updates that ran without them)
    int reload(hipStream_t stream) {
        HIP_TRY(hipMemcpyAsync(h_min.p, d_min.p, n * sizeof(float), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        fill_mirrors(mirror());
        return PQV_OK;
    }
    // total = sum over worker chunks of the chunk's sequential f32 sum (:356-370).  Each chunk's sum is its own sequential f32
    // chain and the chains are independent of each other: they run side by side -- one per vector lane over the transposed mirror,
    // else eight full chunks at a time, else one by one; the chunk sums still join `total` in ascending chunk order.
    float total() {
        const float *md = mirror();
        float total = 0.0f;
        uint64_t s = 0;
        if (use_t) {
            float *acc = chain_acc.data();
            for (uint64_t c = 0; c < wpad; ++c) acc[c] = 0.0f;
            chain_sums(h_min_t.as<float>(), chunk, wpad, acc);
            for (uint64_t c = 0; c < n_chunks; ++c) total = total + acc[c];
            s = n;
        } else if (chunk < n) {
            for (; s + 8 * chunk <= n; s += 8 * chunk) {
                const float *p = md + s;
                float a0 = 0.0f, a1 = 0.0f, a2 = 0.0f, a3 = 0.0f, a4 = 0.0f, a5 = 0.0f, a6 = 0.0f, a7 = 0.0f;
                for (uint64_t t = 0; t < chunk; ++t) {
                    a0 = a0 + p[t];             a1 = a1 + p[chunk + t];     a2 = a2 + p[2 * chunk + t]; a3 = a3 + p[3 * chunk + t];
                    a4 = a4 + p[4 * chunk + t]; a5 = a5 + p[5 * chunk + t]; a6 = a6 + p[6 * chunk + t]; a7 = a7 + p[7 * chunk + t];
                }
                total = total + a0; total = total + a1; total = total + a2; total = total + a3;
                total = total + a4; total = total + a5; total = total + a6; total = total + a7;
            }
        }
        for (; s < n; s += chunk) {
            const uint64_t e = std::min(n, s + chunk);
            float local = 0.0f;
            for (uint64_t t = s; t < e; ++t) local = local + md[t];
            total = total + local;
        }
        return total;
    }
};

// The plain update of the minima (stream_kernel, STREAM_MINUPD): the subset's distances to the row `queries` (set per launch) are
// folded into d_min and both mirrors.
pqv::StreamArgs kpp_minupd_pass(const KppSubset &subset, const KppMinima &minima) {
    pqv::StreamArgs sa{};
    sa.mat = subset.d_init; sa.row_of = nullptr; sa.list_off = nullptr; sa.probe = nullptr; sa.cand_base = nullptr;
    sa.single_begin = 0; sa.single_end = subset.init_n;
    sa.nq = 1; sa.nprobe = 1; sa.dim = subset.dim; sa.k = 1;
    sa.rows_per_block = 256;
    sa.blocks_per_list = static_cast<uint32_t>((subset.init_n + 255) / 256);
    sa.max_pos = ~0ull; sa.metric = PQV_L2SQ_REF4;
    sa.out_f32 = minima.d_min.as<float>();
    sa.mirror_f32 = minima.mirror();
    sa.mirror_t = minima.mirror_t(); sa.mirror_chunk = minima.mirror_chunk; sa.mirror_stride = minima.mirror_stride;
    return sa;
}

// Round 4: from the second measured centroid on, a round first screens the rows with int8 images (minupd_screen_kernel): a row
// whose distance to the new centroid provably is not below its current minimum is not evaluated (after a dozen rounds: most).
// Rows of a multiple of 64 dims, finite data; PQV_KPP_SCREEN=0 keeps the plain streaming pass (A/B, tests).
struct KppRoundScreen {
    DevBuf d_kimg, d_kn2i, d_kres, d_kaux, d_kmm;
    pqv::MinUpdScreenArgs ms{};
    bool applies = false;
    // images the subset; applies = the screen serves these rows, ms is filled
    int init(const KppSubset &subset, const KppMinima &minima, uint32_t k, hipStream_t stream) {
        using namespace pqv;
        const uint64_t init_n = subset.init_n; const uint32_t dim = subset.dim; const float *d_init = subset.d_init;
        if (!(env_on("PQV_KPP_SCREEN") && (dim % 64) == 0 && dim >= 128 && dim <= 8192 && init_n >= 1024 && k > 8)) return PQV_OK;
        const uint64_t n_tiles = (init_n + 15) / 16;
        // one "list" holding the whole subset: {list_off[2], blk_off[2]} u64, then centre[dim], half, scale, radius floats
        HIP_TRY(d_kaux.alloc(4 * sizeof(uint64_t) + (static_cast<size_t>(dim) + 3) * sizeof(float)));
        const uint64_t h_off[4] = {0, init_n, 0, n_tiles};
        HIP_TRY(hipMemcpyAsync(d_kaux.p, h_off, sizeof h_off, hipMemcpyHostToDevice, stream));
        const uint64_t *d_loff = d_kaux.as<uint64_t>(), *d_boff = d_loff + 2;
        float *d_ctr = reinterpret_cast<float *>(d_kaux.as<uint64_t>() + 4), *d_half = d_ctr + dim, *d_scale = d_half + 1, *d_rad = d_scale + 1;
        HIP_TRY(d_kmm.alloc(2 * static_cast<size_t>(dim) * sizeof(uint32_t)));
        uint32_t *kmin = d_kmm.as<uint32_t>(), *kmax = kmin + dim;
        HIP_TRY(hipMemsetAsync(kmin, 0xFF, static_cast<size_t>(dim) * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(kmax, 0, static_cast<size_t>(dim) * sizeof(uint32_t), stream));
        HIP_TRY(d_kimg.alloc(n_tiles * 16 * dim));
        HIP_TRY(d_kn2i.alloc(init_n * sizeof(int)));
        HIP_TRY(d_kres.alloc(init_n * sizeof(float)));
        HIP_TRY(launch_list_minmax(d_init, d_loff, 1, init_n, dim, kmin, kmax, stream));
        HIP_TRY(launch_list_center(kmin, kmax, 1, dim, d_loff, d_ctr, d_half, d_scale, d_rad, stream));
        HIP_TRY(launch_block_rows_i8(d_init, d_loff, d_boff, 1, n_tiles, dim, d_ctr, d_scale, d_half, d_rad, d_kimg.p, d_kn2i.as<int>(),
                                     d_kres.as<float>(), stream));
        float h_hs[2] = {0.0f, 0.0f};       // {half range, scale}
        HIP_TRY(hipMemcpyAsync(h_hs, d_half, sizeof h_hs, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        // (a non-finite value anywhere in the subset shows in the half range; a degenerate scale -- all rows equal -- has nothing to screen)
        if (!(h_hs[0] > 0.0f && h_hs[0] < 1.0e30f && h_hs[1] > 1.0e-30f && h_hs[1] < 1.0e15f)) return PQV_OK;
        ms.rows = d_init; ms.img = static_cast<const float4 *>(d_kimg.p); ms.n2i = d_kn2i.as<int>(); ms.res = d_kres.as<float>();
        ms.n = init_n; ms.dim = dim; ms.inv_s = 1.0f / h_hs[1];
        ms.cm = static_cast<float>(dim + 16) * 2.384185791015625e-07f;
        ms.min_d = minima.d_min.as<float>(); ms.mirror = minima.mirror();
        ms.mirror_t = minima.mirror_t(); ms.mirror_chunk = minima.mirror_chunk; ms.mirror_stride = minima.mirror_stride;
        applies = true;
        return PQV_OK;
    }
    void release() { d_kimg.release(); d_kn2i.release(); d_kres.release(); d_kaux.release(); d_kmm.release(); }
};

// The scratch of kpp_pick_kernel, one zeroed block: picks [n_picks] | chunk sums [n_chunks] | block sums [64] | quarter-run pairs
// [4096] | block flags [64] | head [72] (u64 each), then draws [n_draws] f32, state [4] u32 and, where asked for, 16-byte aligned
// minima [n_minima] f32 (pqv_kpp_pick's copy of them: aligned as the build's d_min is).
struct KppScratch {
    DevBuf buf;
    float *draws = nullptr, *minima = nullptr;
    pqv::KppPickArgs pa{};         // picks, state, draws (u) and the sums' pointers over the block; md, n, chunk and round are the caller's
    // stream: where the zero fill is enqueued; nullptr: the blocking hipMemset (pqv_kpp_pick has no stream of its own)
    int init(size_t n_picks, size_t n_draws, uint64_t n_chunks, size_t n_minima, const hipStream_t *stream) {
        const size_t n64 = n_picks + n_chunks + 64 + 4096 + 64 + 72;
        const size_t bytes = n64 * 8 + (n_draws + 4) * 4 + (n_minima ? 16 + n_minima * 4 : 0);
        HIP_TRY(buf.alloc(bytes));
        if (stream) HIP_TRY(hipMemsetAsync(buf.p, 0, bytes, *stream));
        else HIP_TRY(hipMemset(buf.p, 0, bytes));
        pa.picks = buf.as<unsigned long long>(); pa.n_chunks = static_cast<uint32_t>(n_chunks);
        pa.chunk_sum = pa.picks + n_picks; pa.blk_sum = pa.chunk_sum + n_chunks; pa.run_sum = pa.blk_sum + 64; pa.blk_done = pa.run_sum + 4096;
        pa.head = pa.blk_done + 64;
        pa.u = draws = reinterpret_cast<float *>(pa.picks + n64);
        pa.state = reinterpret_cast<uint32_t *>(draws + n_draws);
        if (n_minima) minima = reinterpret_cast<float *>((reinterpret_cast<uintptr_t>(pa.state + 4) + 15) & ~static_cast<uintptr_t>(15));
        return PQV_OK;
    }
};

// (Measured and dropped: the screened rounds as ONE resident kernel fed through pinned memory -- commands polled with relaxed
//  system-scope loads, minima mirrored with system-scope stores, a ticket per block -- 45 us a round against 24 for a launch per
//  round: the PCIe round trips of the hand-shake cost more than a kernel launch and its completion.  Likewise a completion flag
//  written by the last block of a per-round launch: the per-block system-scope release costs the kernel 20 us.)
// Round 6: the rounds enqueued ahead with the pick on the device (kernels_kpp.hip: the reference's sequential f32 sums evaluated
// exactly by composing the additions' integer images) -- no host round trip per centroid.  The draws of :373 are taken from a copy
// of the generator (one per round while every total is positive); a round the device cannot decide the reference's way stops the
// chain and the host walk takes over from that round.  PQV_KPP_DEVICE=0 keeps the host walk for every round (A/B, tests).
// sa: the plain pass against centroid 0 (round 1's update).  *decided = the first round left to the host (k: none): picks[1 ..
// decided) are set, rng has made their draws and, where rounds are left, the minima's mirrors are the device's state behind round
// `decided`'s update (the chain ran without them).
int kpp_device_rounds(pqv::StdRng &rng, const pqv::StreamArgs &sa, const pqv::MinUpdScreenArgs &ms, KppMinima &minima, uint32_t k,
                      std::vector<uint64_t> &picks, hipStream_t stream, uint32_t *decided_out) {
    using namespace pqv;
    const double t_d0 = now_s();
    KppScratch scratch;
    if (int rc = scratch.init(k, k, minima.n_chunks, 0, &stream)) return rc;
    StdRng ahead = rng;
    std::vector<float> draws(k, 0.0f);
    for (uint32_t i = 1; i < k; ++i) draws[i] = ahead.unit_f32();
    const unsigned long long pick0 = picks[0];
    HIP_TRY(hipMemcpyAsync(scratch.pa.picks, &pick0, sizeof pick0, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(scratch.draws, draws.data(), static_cast<size_t>(k) * sizeof(float), hipMemcpyHostToDevice, stream));
    StreamArgs sd = sa;
    sd.mirror_f32 = nullptr; sd.mirror_t = nullptr;
    HIP_TRY(launch_stream(sd, STREAM_MINUPD, stream));
    MinUpdScreenArgs md_args = ms;
    md_args.mirror = nullptr; md_args.mirror_t = nullptr; md_args.stop = scratch.pa.state;
    KppPickArgs pa = scratch.pa;
    pa.md = minima.d_min.as<float>(); pa.n = static_cast<uint32_t>(minima.n); pa.chunk = static_cast<uint32_t>(minima.chunk);
    for (uint32_t i = 1; i < k; ++i) {
        if (i > 1) {                                   // (round 1 would re-measure centroid 0)
            md_args.pick_dev = scratch.pa.picks + (i - 1);
            HIP_TRY(launch_minupd_screen(md_args, stream));
        }
        pa.round = i;
        HIP_TRY(launch_kpp_pick(pa, stream));
    }
    uint32_t h_state[4] = {0, 0, 0, 0};
    std::vector<unsigned long long> h_picks(k, ~0ull);
    HIP_TRY(hipMemcpyAsync(h_picks.data(), scratch.pa.picks, static_cast<size_t>(k) * sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(h_state, scratch.pa.state, sizeof h_state, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint32_t decided = h_state[0] ? std::min<uint32_t>(std::max<uint32_t>(h_state[1], 1), k) : k;   // rounds 1 .. decided - 1
    for (uint32_t i = 1; i < decided; ++i) picks[i] = h_picks[i];
    for (uint32_t i = 1; i < decided; ++i) (void)rng.unit_f32();     // the generator follows the rounds that were decided
    if (verbose()) std::fprintf(stderr, "[pqv] k-means++ on the device: rounds 1..%u of %u in %.1f ms%s\n", decided - 1, k - 1,
                                (now_s() - t_d0) * 1e3, h_state[0] ? " (the host walk takes over)" : "");
    if (decided < k) {
        if (verbose()) std::fprintf(stderr, "[pqv] k-means++: round %u back to the host (reason %u)\n", decided, h_state[2]);
        if (int rc = minima.reload(stream)) return rc;
    }
    *decided_out = decided;
    return PQV_OK;
}

// Rounds i_start .. k - 1 on the host (:354-390): a round's one command updates the minima against centroid i - 1, the host adds
// the chunk sums off the mirror and walks to the pick.  Round i_start's update has run before the call -- round 1's is the plain
// pass against centroid 0, a later one the device chain's last -- so the first round here launches nothing.
int kpp_host_rounds(pqv::StdRng &rng, uint32_t i_start, uint32_t k, const KppSubset &subset, KppMinima &minima, pqv::StreamArgs sa,
                    KppRoundScreen &screen, const float *d_centroids, std::vector<uint64_t> &picks, hipStream_t stream) {
    using namespace pqv;
    const uint64_t init_n = subset.init_n;
    double tt_gpu = 0.0, tt_sum = 0.0, tt_pick = 0.0;       // PQV_VERBOSE: where a round's time goes
    const bool vb = verbose();
    // round 6: the pick's walk starts on a second host thread while this one adds the chunk sums (PrefixScout; PQV_KPP_SCOUT=0: one thread)
    std::unique_ptr<PrefixScout> scout;
    if (env_on("PQV_KPP_SCOUT") && std::thread::hardware_concurrency() >= 2 && k > 2 && init_n >= 4096 && i_start < k) {
        scout.reset(new (std::nothrow) PrefixScout());
        if (scout) scout->start(minima.mirror(), init_n);
    }
    for (uint32_t i = i_start; i < k; ++i) {
        const double tr0 = vb ? now_s() : 0.0;
        if (i > i_start) {
            if (screen.applies && picks[i - 1] != ~0ull) {
                screen.ms.pick = picks[i - 1];
                HIP_TRY(launch_minupd_screen(screen.ms, stream));
            } else {                                                // (a centroid that is no subset row -- the zero fill -- takes the plain pass)
                sa.queries = picks[i - 1] != ~0ull ? subset.row(picks[i - 1]) : d_centroids + static_cast<uint64_t>(i - 1) * subset.dim;
                HIP_TRY(launch_stream(sa, STREAM_MINUPD, stream));
            }
        }
        {
            // the round's only command: poll for its completion (the blocking wait's wake-up costs several microseconds a round)
            hipError_t qe;
            uint32_t polls = 0;
            while ((qe = hipStreamQuery(stream)) == hipErrorNotReady && ++polls < 200000u) { }
            if (qe != hipSuccess) { (void)hipGetLastError(); HIP_TRY(hipStreamSynchronize(stream)); }
        }
        const double tr1 = vb ? now_s() : 0.0;
        if (scout) scout->begin(i);
        const float *md = minima.mirror();
        const float total = minima.total();
        const double tr2 = vb ? now_s() : 0.0;
        if (total > 0.0f) {
            const float threshold = rng.unit_f32() * total;                            // :373
            if (scout) {
                picks[i] = scout->finish(i, threshold, false);                         // (~0: no slot reached it, as below)
            } else {
                float cumsum = 0.0f;
                for (uint64_t slot = 0; slot < init_n; ++slot) {                       // :375-383
                    cumsum = cumsum + md[slot];
                    if (cumsum >= threshold) { picks[i] = slot; break; }
                }
            }
        } else {
            if (scout) (void)scout->finish(i, 0.0f, true);
            picks[i] = rng.range_usize(0, init_n);                                     // :385
        }
        if (vb) { const double tr3 = now_s(); tt_gpu += tr1 - tr0; tt_sum += tr2 - tr1; tt_pick += tr3 - tr2; }
    }
    if (vb) std::fprintf(stderr, "[pqv] k-means++ rounds: launch + wait %.1f ms, chunk sums %.1f ms, pick scan %.1f ms\n", tt_gpu * 1e3, tt_sum * 1e3, tt_pick * 1e3);
    return PQV_OK;
}

// the chosen rows -> the centroid table (a centroid without a pick keeps its zero fill, as in the reference)
int kpp_commit(const std::vector<uint64_t> &picks, const KppSubset &subset, float *d_centroids, hipStream_t stream) {
    const uint32_t k = static_cast<uint32_t>(picks.size()), dim = subset.dim;
    bool all = true;
    for (uint32_t i = 0; i < k; ++i) all = all && picks[i] != ~0ull;
    if (all) {
        DevBuf d_picks;
        HIP_TRY(d_picks.alloc(static_cast<size_t>(k) * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(d_picks.p, picks.data(), static_cast<size_t>(k) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(pqv::launch_gather_rows(subset.d_init, nullptr, d_picks.as<uint64_t>(), k, dim, d_centroids, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    } else {
        for (uint32_t i = 0; i < k; ++i)
            if (picks[i] != ~0ull)
                HIP_TRY(hipMemcpyAsync(d_centroids + static_cast<uint64_t>(i) * dim, subset.row(picks[i]), dim * sizeof(float),
                                       hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return PQV_OK;
}

// Lloyd iterations (:392-454) over d_data [n, dim] from the centroids k-means++ left in d_centroids.  t0: the clock origin of the
// phase (the end of k-means++).
int lloyd_iterations(const float *d_data, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iters, hipStream_t stream, float *d_centroids,
                     double t0, std::vector<uint32_t> *assign_out, uint32_t *iters_run) {
    using namespace pqv;
    DevBuf d_assign_a, d_assign_b, d_counts, d_list_rows, d_list_off;
    HIP_TRY(d_assign_a.alloc(n * sizeof(uint32_t)));
    HIP_TRY(d_assign_b.alloc(n * sizeof(uint32_t)));
    HIP_TRY(d_counts.alloc((static_cast<size_t>(k) + 1) * sizeof(unsigned long long)));
    HIP_TRY(d_list_rows.alloc(n * sizeof(uint32_t)));
    HIP_TRY(d_list_off.alloc((static_cast<size_t>(k) + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMemsetAsync(d_assign_a.p, 0, n * sizeof(uint32_t), stream));            // :392
    uint32_t *d_prev = d_assign_a.as<uint32_t>(), *d_cur = d_assign_b.as<uint32_t>();
    std::vector<uint32_t> h_assign(n, 0);
    std::vector<unsigned long long> h_counts(static_cast<size_t>(k) + 1);
    std::vector<uint64_t> off;
    std::vector<uint32_t> rows;
    uint32_t iters = 0;
    // Lloyd tries ONE tier above the exact kernel: the contraction where it applies, else the screen, never the screen behind a
    // contraction that stepped down.  What makes a tier step down -- a non-finite row, a centroid that is one -- is there again in
    // the next iteration, and a second tier would spend its norm passes and its synchronisation on it every time; assign_rows
    // runs once and does try both.
    AssignLadder ladder;
    ladder.try_gemm = GemmAssign::applicable(dim, k);
    ladder.try_screen = !ladder.try_gemm && ScreenedAssign::applicable(dim, k);
    ladder.gemm.keep_mu = env_on("PQV_LLOYD_KEEP_IMAGES");
    const bool dev_lists = DeviceLists::applicable(n, k);
    DeviceLists dlists;
    uint32_t h_bad = 0;
    if (dev_lists) {
        if (int rc = dlists.prepare(n, k)) return rc;
        HIP_TRY(hipMemsetAsync(dlists.bad.p, 0, sizeof(uint32_t), stream));
    }
    for (uint32_t iter = 0; iter < max_iters; ++iter) {
        HIP_TRY(hipMemsetAsync(d_counts.p, 0, (static_cast<size_t>(k) + 1) * sizeof(unsigned long long), stream));
        unsigned long long *d_changed = d_counts.as<unsigned long long>() + k;
        AssignLadder::Tier tier;
        if (int rc = ladder.run(d_data, n, d_centroids, k, dim, d_cur, stream, &tier, d_prev, d_changed)) return rc;
        HIP_TRY(hipMemcpyAsync(h_counts.data(), d_counts.p, h_counts.size() * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, stream));
        if (!dev_lists) HIP_TRY(hipMemcpyAsync(h_assign.data(), d_cur, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (dev_lists && iter > 0)                 // (the previous iteration's range check rides on this synchronisation)
            HIP_TRY(hipMemcpyAsync(&h_bad, dlists.bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h_bad) return fail(PQV_ERR_HIP, "internal error: Lloyd assignment out of range");
        iters++;
        std::swap(d_prev, d_cur);
        if (h_counts[k] == 0) break;                                                   // :432
        if (dev_lists) {
            if (int rc = dlists.run(d_prev, n, k, d_list_off.as<uint64_t>(), d_list_rows.as<uint32_t>(), stream)) return rc;
        } else {
            if (!lists_from_assignment(h_assign.data(), n, k, off, rows))
                return fail(PQV_ERR_HIP, "internal error: Lloyd assignment out of range");
            HIP_TRY(hipMemcpyAsync(d_list_off.p, off.data(), off.size() * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
            HIP_TRY(hipMemcpyAsync(d_list_rows.p, rows.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        }
        HIP_TRY(launch_lloyd_update(d_data, dim, d_list_rows.as<uint32_t>(), d_list_off.as<uint64_t>(),
                                    k, d_centroids, stream));                          // :436-453
    }
    if (dev_lists && iters > 0) {
        HIP_TRY(hipMemcpyAsync(&h_bad, dlists.bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        if (assign_out) HIP_TRY(hipMemcpyAsync(h_assign.data(), d_prev, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipStreamSynchronize(stream));
    if (h_bad) return fail(PQV_ERR_HIP, "internal error: Lloyd assignment out of range");
    g_build_stats[BS_LLOYD_S] = now_s() - t0; g_build_stats[BS_ITERS] = iters;
    g_build_stats[BS_LLOYD_FORM] = ladder.try_gemm ? AssignLadder::GEMM : ladder.try_screen ? AssignLadder::SCREEN : AssignLadder::EXACT;
    if (verbose()) std::fprintf(stderr, "[pqv] Lloyd: %u iterations over %llu rows in %.3f s\n", iters,
                                (unsigned long long)n, now_s() - t0);
    if (iters_run) *iters_run = iters;
    if (assign_out) *assign_out = std::move(h_assign);
    return PQV_OK;
}

// d_data [n, dim] resident; writes d_centroids [k, dim] (device) and optionally the final
// assignment (host).
int kmeans_device(const float *d_data, uint64_t n, uint32_t dim, uint32_t k, uint32_t max_iters,
                  uint64_t seed, uint32_t workers, hipStream_t stream, float *d_centroids,
                  std::vector<uint32_t> *assign_out, uint32_t *iters_run) {
    using namespace pqv;
    if (workers == 0) workers = host_workers();
    StdRng rng = StdRng::seed_from_u64(seed);                                          // :327
    HIP_TRY(hipMemsetAsync(d_centroids, 0, static_cast<size_t>(k) * dim * sizeof(float), stream)); // :330

    // k-means++ (:332-390).  Centroid i is row picks[i] of the subset (~0: none, the centroid keeps its zero fill).  A round measures
    // against that row where it lies and the rows are copied into the table once, after the last round, so that a round is ONE command
    // on the stream: no device-to-device copy before its kernel, no download after it (the kernel mirrors the minima into pinned host
    // memory): 83 -> 64 us per round on C3's 50 000 x 768 subset (kernel 26 us, the host scans about 20).
    KppSubset subset;
    if (int rc = subset.draw(rng, d_data, n, dim, k, stream)) return rc;
    std::vector<uint64_t> picks(k, ~0ull);
    picks[0] = rng.range_usize(0, subset.init_n);                                      // :340-342
    KppMinima minima;
    if (int rc = minima.init(subset.init_n, workers, stream)) return rc;
    StreamArgs sa = kpp_minupd_pass(subset, minima);
    const double t_pp0 = now_s();
    KppRoundScreen screen;
    if (int rc = screen.init(subset, minima, k, stream)) return rc;
    sa.queries = subset.row(picks[0]);             // distances to centroid 0
    uint32_t i_start = 1;
    if (env_on("PQV_KPP_DEVICE") && screen.applies && k >= 3 && minima.n <= 57344 && minima.n_chunks <= 1024 && minima.chunk <= 0xFFFFFFFFull) {
        if (int rc = kpp_device_rounds(rng, sa, screen.ms, minima, k, picks, stream, &i_start)) return rc;
    } else {
        HIP_TRY(launch_stream(sa, STREAM_MINUPD, stream));
    }
    if (int rc = kpp_host_rounds(rng, i_start, k, subset, minima, sa, screen, d_centroids, picks, stream)) return rc;
    if (int rc = kpp_commit(picks, subset, d_centroids, stream)) return rc;
    HIP_TRY(hipStreamSynchronize(stream));
    minima.d_min.release(); subset.release(); screen.release();
    HIP_TRY(hipStreamSynchronize(stream));
    const double t_pp1 = now_s();
    g_build_stats[BS_KPP_S] = t_pp1 - t_pp0; g_build_stats[BS_WIDE_KERNEL_S] = 0.0; g_build_stats[BS_WIDE_LAUNCHES] = 0.0;
    if (verbose()) std::fprintf(stderr, "[pqv] k-means++: %u rounds over %llu rows in %.3f s\n", k,
                                (unsigned long long)subset.init_n, t_pp1 - t_pp0);

    return lloyd_iterations(d_data, n, dim, k, max_iters, stream, d_centroids, t_pp1, assign_out, iters_run);
}

// The final-assignment stage (index.rs:189-201 + :244-257): d_cluster[i] = nearest_centroid of row i of d_rows [n, dim] under
// d_centroids [k, dim], i in [0, n), by the ladder with both tiers above the exact kernel where they apply: one call over all the
// rows, so the screen behind a contraction that stepped down is one more pass, paid once (Lloyd chooses differently: see there).
// Depends on the centroids and these rows alone: the build calls it over the whole column, pqv_index_assign / pqv_index_append
// over a row range (d_rows = the range's first row: the three forms index rows and outputs from the base they are given and ask
// no more alignment of it than a row start has -- 16 bytes where dim % 4 == 0, the scalar loads of the exact kernel otherwise;
// the non-finite checks read the norms of these n rows only).
// time_kernels: the build's HIP-event bracket of the contraction kernel (BS_WIDE_KERNEL_S, BS_WIDE_LAUNCHES).  t0: the caller's
// clock origin of the PQV_VERBOSE lines.  *decided: the tier that wrote d_cluster.
int assign_rows(const float *d_rows, uint64_t n, uint32_t dim, const float *d_centroids, uint32_t k, uint32_t *d_cluster,
                hipStream_t stream, bool time_kernels, double t0, AssignLadder::Tier *decided) {
    AssignLadder ladder;
    ladder.try_gemm = GemmAssign::applicable(dim, k);
    ladder.try_screen = ScreenedAssign::applicable(dim, k);
    ladder.one_shot = true; ladder.t0 = t0;
    ladder.gemm.time_kernels = time_kernels;
    return ladder.run(d_rows, n, d_centroids, k, dim, d_cluster, stream, decided);
}

// PQV_KEEP_DEVICE_LISTS=0: a built or derived index' lists are downloaded at once instead of staying on the device
bool keep_device_lists() {
    static const bool keep = env_on("PQV_KEEP_DEVICE_LISTS");
    return keep;
}
// The sorted row ids stay where they are: a searcher on this device copies them device to device, and the host copy (40 MB per
// 10 M rows: 3.5 ms of download) is made by the first call that reads it (ListRows::get).
void adopt_device_lists(pqv_index *idx, DevBuf &rows, int device, uint64_t n) {
    auto dr = std::make_shared<DevRows>();
    dr->p = rows.p; dr->device = device; dr->n = n;
    rows.p = nullptr; rows.bytes = 0;
    idx->rows->dev = std::move(dr);
    idx->rows->n = n;
    idx->rows->host.clear();
    idx->rows->pending = true;
}

int build_index_impl(const pqv_corpus *corpus, uint32_t n_clusters, uint32_t max_iters,
                     uint64_t seed, uint32_t workers, pqv_index **out) {
    using namespace pqv;
    const uint64_t n = corpus->n;
    const uint32_t dim = corpus->dim;
    if (max_iters == 0) return fail(PQV_ERR_INVALID, "max_iters must be > 0");         // parquet.rs:90
    if (n == 0) return fail(PQV_ERR_INVALID, "Cannot build IVF index with zero vectors"); // index.rs:158
    uint64_t k = n_clusters;
    if (k == 0) k = static_cast<uint64_t>(std::ceil(std::sqrt(static_cast<double>(n)))); // :164
    if (k > n) return fail(PQV_ERR_INVALID, "n_clusters cannot exceed number of vectors"); // :169
    if (k > 0xFFFFFFFFull) return fail(PQV_ERR_INVALID, "Cluster count must fit in u32");
    if (!corpus->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    if (int rc = use_device(corpus->device)) return rc;
    hipStream_t stream = corpus->stream;
    g_build_stats[BS_WIDE_KERNEL_S] = 0.0; g_build_stats[BS_WIDE_LAUNCHES] = 0.0;      // (kernel seconds / launches of THIS build's final assignment, whichever path it takes)

    uint64_t sample_size = std::max<uint64_t>(n / 20, 1);                              // :172
    sample_size = std::min<uint64_t>(sample_size, 100000);                             // :173
    sample_size = std::min<uint64_t>(std::max<uint64_t>(sample_size, k), n);           // :174

    const double t_b0 = now_s();
    DevBuf d_centroids, d_sample, d_idx;
    HIP_TRY(d_centroids.alloc(k * dim * sizeof(float)));
    const float *d_train = corpus->d_rows;
    if (sample_size != n) {                                                            // :182-187
        StdRng rng = StdRng::seed_from_u64(seed);                                      // :231
        std::vector<uint64_t> idx = index_sample(rng, n, sample_size);                 // :232
        if (verbose()) std::fprintf(stderr, "[pqv] build: sample indices drawn at %.1f ms\n", (now_s() - t_b0) * 1e3);
        HIP_TRY(d_idx.alloc(sample_size * sizeof(uint64_t)));
        HIP_TRY(d_sample.alloc(sample_size * dim * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(d_idx.p, idx.data(), sample_size * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(launch_gather_rows(corpus->d_rows, nullptr, d_idx.as<uint64_t>(), sample_size, dim,
                                   d_sample.as<float>(), stream));
        HIP_TRY(hipStreamSynchronize(stream));
        d_train = d_sample.as<float>();
    }
    const double t_b1 = now_s();
    if (int rc = kmeans_device(d_train, sample_size, dim, static_cast<uint32_t>(k), max_iters, seed,
                               workers, stream, d_centroids.as<float>(), nullptr, nullptr))
        return rc;
    const double t_b2 = now_s();
    d_sample.release(); d_idx.release();
    if (verbose()) std::fprintf(stderr, "[pqv] build: training sample %.3f s, k-means call %.3f s (k-means++ %.3f + Lloyd %.3f inside)\n",
                                t_b1 - t_b0, t_b2 - t_b1, g_build_stats[BS_KPP_S], g_build_stats[BS_LLOYD_S]);

    // final assignment of every row (:189-206)
    const double t_fa0 = now_s();
    DevBuf d_cluster;
    HIP_TRY(d_cluster.alloc(n * sizeof(uint32_t)));
    // The two host arrays of n row ids (the downloaded assignment and the lists) are allocated and first-touched by a
    // helper thread while the device assigns: 2 x 40 MB of page faults on C3 that used to follow the kernels.
    std::vector<uint32_t> cluster_of, rows_buf;
    const bool dev_lists = DeviceLists::applicable(n, static_cast<uint32_t>(k));      // (the lists sorted on the device: no assignment download)
    struct Joiner { std::thread t; ~Joiner() { if (t.joinable()) t.join(); } } warm;
    if (n >= (1u << 20)) {
        try {
            warm.t = std::thread([&cluster_of, &rows_buf, n, dev_lists] {
                try { if (!dev_lists) { cluster_of.resize(n); rows_buf.resize(n); } } catch (...) { }
            });
        } catch (const std::system_error &) { }
    }
    AssignLadder::Tier assign_tier = AssignLadder::EXACT;
    if (int rc = assign_rows(corpus->d_rows, n, dim, d_centroids.as<float>(), static_cast<uint32_t>(k), d_cluster.as<uint32_t>(), stream,
                             true, t_fa0, &assign_tier))
        return rc;
    // the lists: sorted on the device (the rows of a list ascending, index.rs:193-206), then ONE download of the sorted row ids
    // in place of the assignment's download + the host threads' counting sort
    DeviceLists dlists;
    DevBuf d_rows_sorted, d_off;
    if (dev_lists) {
        if (int rc = dlists.prepare(n, static_cast<uint32_t>(k))) return rc;
        HIP_TRY(d_rows_sorted.alloc(n * sizeof(uint32_t)));
        HIP_TRY(d_off.alloc((k + 1) * sizeof(uint64_t)));
        if (int rc = dlists.run(d_cluster.as<uint32_t>(), n, static_cast<uint32_t>(k), d_off.as<uint64_t>(), d_rows_sorted.as<uint32_t>(), stream))
            return rc;
    }
    if (verbose()) { HIP_TRY(hipStreamSynchronize(stream)); std::fprintf(stderr, "[pqv] final assignment: lists sorted at %.1f ms\n", (now_s() - t_fa0) * 1e3); }
    if (warm.t.joinable()) warm.t.join();
    if (verbose()) std::fprintf(stderr, "[pqv] final assignment: host arrays ready at %.1f ms\n", (now_s() - t_fa0) * 1e3);
    if (!dev_lists) cluster_of.resize(n);
    pqv_index *idx = new (std::nothrow) pqv_index();
    if (!idx) return fail(PQV_ERR_OOM, "host allocation failed");
    idx->list_rows = std::move(rows_buf);
    idx->dim = dim; idx->n_clusters = static_cast<uint32_t>(k);
    idx->centroids.resize(k * dim);
    uint32_t h_bad = 0;
    hipError_t e = hipSuccess;
    const bool keep_dev = keep_device_lists();
    if (dev_lists) {
        idx->list_off.resize(k + 1);
        if (!keep_dev) {                            // (the lists are not left on the device: downloaded here)
            idx->list_rows.resize(n);
            e = hipMemcpyAsync(idx->list_rows.data(), d_rows_sorted.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
        }
        if (e == hipSuccess) e = hipMemcpyAsync(idx->list_off.data(), d_off.p, (k + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream);
        if (e == hipSuccess) e = hipMemcpyAsync(&h_bad, dlists.bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    } else {
        e = hipMemcpyAsync(cluster_of.data(), d_cluster.p, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
    }
    if (e == hipSuccess)
        e = hipMemcpyAsync(idx->centroids.data(), d_centroids.p, k * dim * sizeof(float), hipMemcpyDeviceToHost, stream);
    if (e == hipSuccess) e = hipStreamSynchronize(stream);
    if (e != hipSuccess) {
        delete idx;
        return fail(PQV_ERR_HIP, std::string("final assignment: ") + hipGetErrorString(e));
    }
    const double t_fa1 = now_s();
    if (dev_lists ? h_bad != 0 : !lists_from_assignment(cluster_of.data(), n, idx->n_clusters, idx->list_off, idx->list_rows)) {
        delete idx;
        return fail(PQV_ERR_HIP, "internal error: final assignment out of range");
    }
    if (dev_lists && keep_dev && d_rows_sorted.p) adopt_device_lists(idx, d_rows_sorted, corpus->device, n);   // (PQV_KEEP_DEVICE_LISTS=0: downloaded above)
    idx->permutation_of = n;                        // every row was assigned exactly once
    idx->set_row_bound(n);
    g_build_stats[BS_FINAL_ASSIGN_S] = t_fa1 - t_fa0; g_build_stats[BS_HOST_LISTS_S] = now_s() - t_fa1; g_build_stats[BS_FINAL_FORM] = assign_tier;
    g_build_stats[BS_SAMPLE_ROWS] = static_cast<double>(sample_size);
    if (verbose()) std::fprintf(stderr, "[pqv] final assignment: %llu rows in %.3f s (+ %.3f s host list build)\n",
                                (unsigned long long)n, t_fa1 - t_fa0, now_s() - t_fa1);
    if (verbose()) {
        std::fprintf(stderr, "[pqv] build: %.3f s in all; hipMalloc %u calls %.1f ms, hipFree %u calls %.1f ms (this thread, since the last report)\n",
                     now_s() - t_b0, g_alloc_n, g_alloc_s * 1e3, g_free_n, g_free_s * 1e3);
        g_alloc_s = g_free_s = 0.0; g_alloc_n = g_free_n = 0;
    }
    *out = idx;
    return PQV_OK;
}

}  // namespace

static int pqv_index_build_impl(const pqv_corpus *corpus, uint32_t n_clusters, uint32_t max_iters,
                               uint64_t seed, uint32_t workers, pqv_index **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!corpus) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
    return build_index_impl(corpus, n_clusters, max_iters, seed, workers, out);
}
extern "C" int pqv_index_build(const pqv_corpus *corpus, uint32_t n_clusters, uint32_t max_iters,
                               uint64_t seed, uint32_t workers, pqv_index **out) {
    return guard([&] { return pqv_index_build_impl(corpus, n_clusters, max_iters, seed, workers, out); });
}

// ---------------------------------------------------------------------------------------
// pqv_index_assign / pqv_index_append: rows that arrived after the build join the index under its centroids
// (index.rs:189-206 + :244-257 for those centroids over the longer column; no k-means)
// ---------------------------------------------------------------------------------------
namespace {

// the checks the two calls share, before any device work
int check_row_range(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows) {
    if (index->dim != corpus->dim)
        return fail(PQV_ERR_INVALID, "index dimension " + std::to_string(index->dim) +
                                         " does not match corpus dimension " + std::to_string(corpus->dim));
    if (n_rows > corpus->n || first_row > corpus->n - n_rows)
        return fail(PQV_ERR_INVALID, "rows [" + std::to_string(first_row) + ", " + std::to_string(first_row) + " + " + std::to_string(n_rows) +
                                         ") are out of range for a corpus of " + std::to_string(corpus->n) + " rows");
    if (first_row + n_rows > (1ull << 32)) return fail(PQV_ERR_INVALID, "row ids must fit in u32");
    if (!corpus->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    return PQV_OK;
}

// the index' centroids on the corpus' device + the assignment of the range: d_cluster[i] = cluster of row first_row + i
int assign_range(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows, DevBuf &d_centroids,
                 DevBuf &d_cluster) {
    hipStream_t stream = corpus->stream;
    HIP_TRY(d_centroids.alloc(index->centroids.size() * sizeof(float)));
    HIP_TRY(d_cluster.alloc(n_rows * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(d_centroids.p, index->centroids.data(), index->centroids.size() * sizeof(float), hipMemcpyHostToDevice, stream));
    AssignLadder::Tier tier;
    return assign_rows(corpus->d_rows + first_row * corpus->dim, n_rows, corpus->dim, d_centroids.as<float>(), index->n_clusters,
                       d_cluster.as<uint32_t>(), stream, false, now_s(), &tier);
}

int index_assign_impl(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows, uint32_t *cluster_out) {
    if (!index || !corpus) return fail(PQV_ERR_INVALID, "index/corpus must not be NULL");
    if (!cluster_out) return fail(PQV_ERR_INVALID, "cluster_out must not be NULL");
    if (int rc = check_row_range(index, corpus, first_row, n_rows)) return rc;
    if (n_rows == 0) return PQV_OK;
    if (int rc = use_device(corpus->device)) return rc;
    DevBuf d_centroids, d_cluster;
    if (int rc = assign_range(index, corpus, first_row, n_rows, d_centroids, d_cluster)) return rc;
    HIP_TRY(hipMemcpyAsync(cluster_out, d_cluster.p, n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, corpus->stream));
    HIP_TRY(hipStreamSynchronize(corpus->stream));
    return PQV_OK;
}

struct EventSet { hipEvent_t e[4] = {}; ~EventSet() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); } };

int index_append_impl(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows, pqv_index **out) {
    using namespace pqv;
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!index || !corpus) return fail(PQV_ERR_INVALID, "index/corpus must not be NULL");
    if (int rc = check_row_range(index, corpus, first_row, n_rows)) return rc;
    uint64_t bound = 0;
    if (!index->row_bound(&bound)) return PQV_ERR_HIP;
    if (first_row < bound)
        return fail(PQV_ERR_INVALID, "first_row " + std::to_string(first_row) + " is below the index' row bound " + std::to_string(bound) +
                                         " (largest indexed row id + 1): appended rows must follow every indexed row");
    const uint32_t k = index->n_clusters;
    const uint64_t n_old = index->n_rows(), total = n_old + n_rows;
    std::unique_ptr<pqv_index> idx(new pqv_index());
    idx->dim = index->dim; idx->n_clusters = k;
    idx->centroids = index->centroids;              // bit for bit
    idx->set_row_bound(first_row + n_rows);
    idx->permutation_of = index->permutation_of == first_row ? first_row + n_rows : 0;
    if (n_rows == 0) {                              // a copy
        const std::vector<uint32_t> *rv = index->rows->get();
        if (!rv) return PQV_ERR_HIP;
        idx->list_off = index->list_off;
        idx->list_rows = *rv;
        *out = idx.release();
        return PQV_OK;
    }
    if (int rc = use_device(corpus->device)) return rc;
    hipStream_t stream = corpus->stream;
    // PQV_APPEND_STATS=1 (diagnostic, read per call): the wall time of the two phases (the stream is drained between them), the splice
    // kernel between two HIP events and a plain device-to-device copy of the same bytes behind it, on stderr
    const bool stats = std::getenv("PQV_APPEND_STATS") != nullptr;
    const double t0 = now_s();
    DevBuf d_centroids, d_cluster;
    if (int rc = assign_range(index, corpus, first_row, n_rows, d_centroids, d_cluster)) return rc;
    if (stats) HIP_TRY(hipStreamSynchronize(stream));
    const double t1 = now_s();

    if (!DeviceLists::applicable(n_rows, k)) {
        // more than 4096 clusters (or PQV_DEVICE_LISTS=0): the range's assignment comes to the host, and every list is its old rows
        // followed by its new ones in ascending order -- lists_from_assignment's rule over the range, behind the old lists
        std::vector<uint32_t> cluster_of(n_rows);
        HIP_TRY(hipMemcpyAsync(cluster_of.data(), d_cluster.p, n_rows * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        std::vector<uint64_t> add_off;
        std::vector<uint32_t> add_rows;
        if (!lists_from_assignment(cluster_of.data(), n_rows, k, add_off, add_rows))
            return fail(PQV_ERR_HIP, "internal error: final assignment out of range");
        const std::vector<uint32_t> *rv = index->rows->get();
        if (!rv) return PQV_ERR_HIP;
        idx->list_off.resize(static_cast<size_t>(k) + 1);
        idx->list_rows.resize(total);
        uint32_t *dst = idx->list_rows.data();
        for (uint32_t c = 0; c < k; ++c) {
            const uint64_t ob = index->list_off[c], ol = index->list_off[c + 1] - ob, ab = add_off[c], al = add_off[c + 1] - ab;
            idx->list_off[c] = ob + ab;
            if (ol) std::memcpy(dst + ob + ab, rv->data() + ob, ol * sizeof(uint32_t));
            for (uint64_t i = 0; i < al; ++i) dst[ob + ab + ol + i] = static_cast<uint32_t>(first_row + add_rows[ab + i]);
        }
        idx->list_off[k] = total;
        *out = idx.release();
        return PQV_OK;
    }

    // the range's rows sorted by cluster on the device (ids local to the range), then ONE pass writes the extended lists
    DeviceLists dlists;
    DevBuf d_add_rows, d_add_off, d_old_off, d_old_up, d_out_rows, d_out_off;
    if (int rc = dlists.prepare(n_rows, k)) return rc;
    HIP_TRY(d_add_rows.alloc(n_rows * sizeof(uint32_t)));
    HIP_TRY(d_add_off.alloc((static_cast<size_t>(k) + 1) * sizeof(uint64_t)));
    if (int rc = dlists.run(d_cluster.as<uint32_t>(), n_rows, k, d_add_off.as<uint64_t>(), d_add_rows.as<uint32_t>(), stream)) return rc;
    HIP_TRY(d_old_off.alloc((static_cast<size_t>(k) + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMemcpyAsync(d_old_off.p, index->list_off.data(), (static_cast<size_t>(k) + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    // the old lists: the index' device copy where it lives on this device (a build's or an append's result), else one upload
    const uint32_t *d_old = nullptr;
    std::shared_ptr<DevRows> old_dev = index->rows->dev;          // (kept alive over the kernel)
    if (n_old) {
        if (old_dev && old_dev->p && old_dev->device == corpus->device && old_dev->n == n_old) {
            d_old = static_cast<const uint32_t *>(old_dev->p);
        } else {
            const std::vector<uint32_t> *rv = index->rows->get();
            if (!rv) return PQV_ERR_HIP;
            HIP_TRY(d_old_up.alloc(n_old * sizeof(uint32_t)));
            HIP_TRY(hipMemcpyAsync(d_old_up.p, rv->data(), n_old * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
            d_old = d_old_up.as<uint32_t>();
        }
    }
    HIP_TRY(d_out_rows.alloc(total * sizeof(uint32_t)));
    HIP_TRY(d_out_off.alloc((static_cast<size_t>(k) + 1) * sizeof(uint64_t)));
    EventSet ev;
    DevBuf d_copy;
    if (stats) {
        for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(d_copy.alloc(total * sizeof(uint32_t)));
        HIP_TRY(hipEventRecord(ev.e[0], stream));
    }
    HIP_TRY(launch_list_splice(d_old_off.as<uint64_t>(), d_old, d_add_off.as<uint64_t>(), d_add_rows.as<uint32_t>(), k,
                               static_cast<uint32_t>(first_row), total, d_out_off.as<uint64_t>(), d_out_rows.as<uint32_t>(), stream));
    if (stats) {
        HIP_TRY(hipEventRecord(ev.e[1], stream));
        HIP_TRY(hipEventRecord(ev.e[2], stream));
        HIP_TRY(hipMemcpyAsync(d_copy.p, d_out_rows.p, total * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipEventRecord(ev.e[3], stream));
    }
    uint32_t h_bad = 0;
    const bool keep_dev = keep_device_lists();
    idx->list_off.resize(static_cast<size_t>(k) + 1);
    if (!keep_dev) {
        idx->list_rows.resize(total);
        HIP_TRY(hipMemcpyAsync(idx->list_rows.data(), d_out_rows.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipMemcpyAsync(idx->list_off.data(), d_out_off.p, (static_cast<size_t>(k) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipMemcpyAsync(&h_bad, dlists.bad.p, sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (h_bad != 0) return fail(PQV_ERR_HIP, "internal error: final assignment out of range");
    if (keep_dev) adopt_device_lists(idx.get(), d_out_rows, corpus->device, total);      // as a build leaves them
    if (stats) {
        float ms_splice = 0.0f, ms_copy = 0.0f;
        (void)hipEventElapsedTime(&ms_splice, ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&ms_copy, ev.e[2], ev.e[3]);
        const double bytes = static_cast<double>(total) * sizeof(uint32_t);
        std::fprintf(stderr, "pqv_index_append: %llu rows onto %llu: assignment %.3f ms, lists %.3f ms; splice kernel %.4f ms for %.0f list bytes "
                             "(%.1f GB/s written), device-to-device copy of the same bytes %.4f ms\n",
                     (unsigned long long)n_rows, (unsigned long long)n_old, (t1 - t0) * 1e3, (now_s() - t1) * 1e3, ms_splice, bytes,
                     ms_splice > 0.0f ? bytes / (ms_splice * 1e6) : 0.0, ms_copy);
    }
    *out = idx.release();
    return PQV_OK;
}

// ---------------------------------------------------------------------------------------
// pqv_index_remove* / pqv_index_compact: rows leave the lists (remove), then the corpus (compact).  Both rank over a bitset on
// the device (kernels_remove.hip); a host path leaves the identical result where the device path is not taken.
// ---------------------------------------------------------------------------------------
bool device_lists_on() { return DeviceLists::applicable(1, 1); }       // (PQV_DEVICE_LISTS alone: these paths have no cluster limit)
bool device_usable(int device) {      // (no error text: the caller falls back to the host)
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess) { (void)hipGetLastError(); return false; }
    return device >= 0 && device < count;
}
struct PooledStream {
    int device = -1;
    hipStream_t s = nullptr;
    ~PooledStream() { if (s) pool_put(device, s); }
};

// the parts every derived index shares with its source: dimension, centroids bit for bit
std::unique_ptr<pqv_index> derive_index(const pqv_index *index) {
    std::unique_ptr<pqv_index> idx(new pqv_index());
    idx->dim = index->dim; idx->n_clusters = index->n_clusters;
    idx->centroids = index->centroids;
    return idx;
}
int copy_lists(const pqv_index *index, pqv_index *idx) {
    const std::vector<uint32_t> *rv = index->rows->get();
    if (!rv) return PQV_ERR_HIP;
    idx->list_off = index->list_off;
    idx->list_rows = *rv;
    idx->permutation_of = index->permutation_of;
    return PQV_OK;
}
// the index' lists on `device`: its device copy where it lives there, else one upload (up keeps it)
int device_lists_of(const pqv_index *index, int device, uint64_t n_pos, hipStream_t stream, std::shared_ptr<DevRows> &keep, DevBuf &up,
                    const uint32_t **d_ids) {
    keep = index->rows->dev;
    if (keep && keep->p && keep->device == device && keep->n == n_pos) { *d_ids = static_cast<const uint32_t *>(keep->p); return PQV_OK; }
    const std::vector<uint32_t> *rv = index->rows->get();
    if (!rv) return PQV_ERR_HIP;
    HIP_TRY(up.alloc(n_pos * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(up.p, rv->data(), n_pos * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
    *d_ids = up.as<uint32_t>();
    return PQV_OK;
}

// flags: host bytes (h_flags) or device bytes (d_flags, from_device); validated by the callers
int index_remove_common(const pqv_index *index, int device, const uint8_t *h_flags, const void *d_flags, bool from_device, uint64_t n_flags,
                        hipStream_t user_stream, pqv_index **out) {
    using namespace pqv;
    if (from_device) if (int rc = use_device(device)) return rc;
    uint64_t bound = 0;
    if (!index->row_bound(&bound)) return PQV_ERR_HIP;
    std::unique_ptr<pqv_index> idx = derive_index(index);
    idx->set_row_bound(bound);                       // carried over, not lowered: ids are never reused
    const uint32_t k = index->n_clusters;
    const uint64_t n_pos = index->n_rows();
    const uint64_t nf = std::min(n_flags, bound);    // (no row at or above the bound is indexed)
    if (n_pos == 0 || nf == 0) {                     // nothing can leave: a copy
        if (int rc = copy_lists(index, idx.get())) return rc;
        *out = idx.release();
        return PQV_OK;
    }
    const bool on_device = device_lists_on() && (from_device || device_usable(device));
    if (!on_device) {
        // PQV_DEVICE_LISTS=0, or host flags and no usable device: list c = its rows whose flag byte is zero, order kept
        std::vector<uint8_t> down;
        if (from_device) {
            hipStream_t stream = user_stream;
            down.resize(nf);
            HIP_TRY(hipMemcpyAsync(down.data(), d_flags, nf, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            h_flags = down.data();
        }
        const std::vector<uint32_t> *rv = index->rows->get();
        if (!rv) return PQV_ERR_HIP;
        idx->list_off.assign(static_cast<size_t>(k) + 1, 0);
        idx->list_rows.reserve(n_pos);
        for (uint32_t c = 0; c < k; ++c) {
            for (uint64_t p = index->list_off[c]; p < index->list_off[c + 1]; ++p) {
                const uint32_t r = (*rv)[p];
                if (r >= nf || h_flags[r] == 0) idx->list_rows.push_back(r);
            }
            idx->list_off[c + 1] = idx->list_rows.size();
        }
        if (idx->list_rows.size() == n_pos) idx->permutation_of = index->permutation_of;
        idx->list_rows.shrink_to_fit();
        *out = idx.release();
        return PQV_OK;
    }

    if (!from_device) if (int rc = use_device(device)) return rc;
    PooledStream pooled;
    hipStream_t stream = user_stream;
    if (!from_device) {
        pooled.device = device;
        HIP_TRY(pool_get(device, &pooled.s));
        stream = pooled.s;
    }
    // PQV_REMOVE_STATS=1 (diagnostic, read per call): the compaction kernel between two HIP events and a plain device-to-device
    // copy of the same list bytes behind it, on stderr
    const bool stats = std::getenv("PQV_REMOVE_STATS") != nullptr;
    const double t0 = now_s();
    std::shared_ptr<DevRows> old_dev;
    DevBuf d_up_ids, d_up_flags, d_bits, d_rank, d_tmp, d_old_off, d_new_off, d_out, d_copy;
    const uint32_t *d_ids = nullptr;
    if (int rc = device_lists_of(index, device, n_pos, stream, old_dev, d_up_ids, &d_ids)) return rc;
    const uint8_t *d_f = static_cast<const uint8_t *>(d_flags);
    if (!from_device) {
        HIP_TRY(d_up_flags.alloc(nf));
        HIP_TRY(hipMemcpyAsync(d_up_flags.p, h_flags, nf, hipMemcpyHostToDevice, stream));
        d_f = d_up_flags.as<uint8_t>();
    }
    // bit p of the image = "the row at list position p is flagged" (launch_mask_layout as it is); the kernels behind it read the
    // image inverted: a set bit leaves
    const uint64_t n_words = (n_pos + 63) / 64, n_words_image = n_words + 1;
    HIP_TRY(d_bits.alloc((n_words_image + 1) * sizeof(uint64_t)));
    unsigned long long *d_count = d_bits.as<unsigned long long>() + n_words_image;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    HIP_TRY(launch_mask_layout(d_f, nf, d_ids, n_pos, d_bits.as<uint64_t>(), n_words_image, d_count, stream));
    HIP_TRY(d_rank.alloc((n_words + 1) * sizeof(uint64_t)));
    HIP_TRY(d_tmp.alloc((bit_rank_blocks(n_pos) + 1) * sizeof(uint64_t)));
    HIP_TRY(launch_bit_rank(d_bits.as<uint64_t>(), n_pos, true, d_rank.as<uint64_t>(), d_tmp.as<uint64_t>(), stream));
    uint64_t kept = 0;
    HIP_TRY(hipMemcpyAsync(&kept, d_rank.as<uint64_t>() + n_words, sizeof kept, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (kept > n_pos) return fail(PQV_ERR_HIP, "internal error: more rows kept than indexed");
    if (kept == n_pos) {                             // nothing was removed: a copy
        if (int rc = copy_lists(index, idx.get())) return rc;
        *out = idx.release();
        return PQV_OK;
    }
    const double t1 = now_s();
    HIP_TRY(d_out.alloc(kept * sizeof(uint32_t)));
    HIP_TRY(d_old_off.alloc((static_cast<size_t>(k) + 1) * sizeof(uint64_t)));
    HIP_TRY(d_new_off.alloc((static_cast<size_t>(k) + 1) * sizeof(uint64_t)));
    HIP_TRY(hipMemcpyAsync(d_old_off.p, index->list_off.data(), (static_cast<size_t>(k) + 1) * sizeof(uint64_t), hipMemcpyHostToDevice, stream));
    EventSet ev;
    if (stats) {
        for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(d_copy.alloc(n_pos * sizeof(uint32_t)));
        HIP_TRY(hipEventRecord(ev.e[0], stream));
    }
    HIP_TRY(launch_list_compact(d_ids, n_pos, d_bits.as<uint64_t>(), true, d_rank.as<uint64_t>(), d_out.as<uint32_t>(), stream));
    if (stats) {
        HIP_TRY(hipEventRecord(ev.e[1], stream));
        HIP_TRY(hipEventRecord(ev.e[2], stream));
        HIP_TRY(hipMemcpyAsync(d_copy.p, d_ids, n_pos * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipEventRecord(ev.e[3], stream));
    }
    HIP_TRY(launch_offsets_rank(d_old_off.as<uint64_t>(), k + 1, d_bits.as<uint64_t>(), n_pos, true, d_rank.as<uint64_t>(),
                                d_new_off.as<uint64_t>(), stream));
    idx->list_off.resize(static_cast<size_t>(k) + 1);
    const bool keep_dev = keep_device_lists();
    if (!keep_dev) {
        idx->list_rows.resize(kept);
        if (kept) HIP_TRY(hipMemcpyAsync(idx->list_rows.data(), d_out.p, kept * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(hipMemcpyAsync(idx->list_off.data(), d_new_off.p, (static_cast<size_t>(k) + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    if (idx->list_off[0] != 0 || idx->list_off[k] != kept) return fail(PQV_ERR_HIP, "internal error: list offsets do not add up");
    if (keep_dev) adopt_device_lists(idx.get(), d_out, device, kept);
    if (stats) {
        float ms_k = 0.0f, ms_copy = 0.0f;
        (void)hipEventElapsedTime(&ms_k, ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&ms_copy, ev.e[2], ev.e[3]);
        const double bytes = static_cast<double>(n_pos) * sizeof(uint32_t);
        std::fprintf(stderr, "pqv_index_remove: %llu of %llu rows leave: keep bits + rank %.3f ms, lists %.3f ms; compaction kernel %.4f ms for %.0f "
                             "list bytes read (%.1f GB/s), device-to-device copy of the same bytes %.4f ms\n",
                     (unsigned long long)(n_pos - kept), (unsigned long long)n_pos, (t1 - t0) * 1e3, (now_s() - t1) * 1e3, ms_k, bytes,
                     ms_k > 0.0f ? bytes / (ms_k * 1e6) : 0.0, ms_copy);
    }
    *out = idx.release();
    return PQV_OK;
}

int index_remove_impl(const pqv_index *index, int device, const uint8_t *h_flags, const void *d_flags, bool from_device, uint64_t n_flags,
                      void *hip_stream, pqv_index **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!index) return fail(PQV_ERR_INVALID, "index must not be NULL");
    if (n_flags && !(from_device ? d_flags != nullptr : h_flags != nullptr)) return fail(PQV_ERR_INVALID, "remove must not be NULL");
    if (n_flags > (1ull << 32)) return fail(PQV_ERR_INVALID, "row ids must fit in u32: n_flags must not exceed 2^32");
    return index_remove_common(index, device, h_flags, d_flags, from_device, n_flags, static_cast<hipStream_t>(hip_stream), out);
}

int index_remove_rows_impl(const pqv_index *index, int device, const uint32_t *rows, uint64_t m, pqv_index **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!index) return fail(PQV_ERR_INVALID, "index must not be NULL");
    if (m && !rows) return fail(PQV_ERR_INVALID, "rows must not be NULL");
    // the byte form over max id + 1 flags, cut at the row bound (no row at or above it is indexed)
    uint64_t bound = 0, n_flags = 0;
    if (!index->row_bound(&bound)) return PQV_ERR_HIP;
    for (uint64_t i = 0; i < m; ++i)
        if (rows[i] < bound) n_flags = std::max<uint64_t>(n_flags, static_cast<uint64_t>(rows[i]) + 1);
    std::vector<uint8_t> flags(n_flags, 0);
    for (uint64_t i = 0; i < m; ++i)
        if (rows[i] < n_flags) flags[rows[i]] = 1;
    return index_remove_common(index, device, flags.data(), nullptr, false, n_flags, nullptr, out);
}

int index_compact_impl(const pqv_index *index, const pqv_corpus *corpus, uint64_t capacity_rows, pqv_corpus **corpus_out,
                       pqv_index **index_out, uint32_t *old_row) {
    using namespace pqv;
    if (corpus_out) *corpus_out = nullptr;
    if (index_out) *index_out = nullptr;
    if (!corpus_out || !index_out) return fail(PQV_ERR_INVALID, "corpus_out/index_out must not be NULL");
    if (!index || !corpus) return fail(PQV_ERR_INVALID, "index/corpus must not be NULL");
    if (index->dim != corpus->dim)
        return fail(PQV_ERR_INVALID, "index dimension " + std::to_string(index->dim) +
                                         " does not match corpus dimension " + std::to_string(corpus->dim));
    if (!corpus->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    const uint64_t n = corpus->n, n_pos = index->n_rows();
    const uint32_t dim = corpus->dim;
    if (n_pos > (1ull << 32)) return fail(PQV_ERR_INVALID, "row ids must fit in u32");
    if (int rc = use_device(corpus->device)) return rc;
    hipStream_t stream = corpus->stream;
    // PQV_REMOVE_STATS=1: the gather kernel between two HIP events and a plain device-to-device copy of the same row bytes
    const bool stats = std::getenv("PQV_REMOVE_STATS") != nullptr;
    const double t0 = now_s();
    std::unique_ptr<pqv_index> idx = derive_index(index);
    idx->list_off = index->list_off;                 // (the rank is applied element by element: every list keeps its length)
    DevBuf d_old_row, d_new_rows;
    uint64_t total = 0;
    const char *const dup_text = "index holds a row more than once: it cannot be compacted";
    const char *const range_text = "index row id out of range for this corpus";
    if (n_pos == 0) {
        HIP_TRY(d_old_row.alloc(16));
    } else if (!device_lists_on()) {
        // PQV_DEVICE_LISTS=0: membership, rank and the renumbered lists on the host; only the rows are gathered on the device
        const std::vector<uint32_t> *rv = index->rows->get();
        if (!rv) return PQV_ERR_HIP;
        std::vector<uint8_t> member(n, 0);
        for (uint32_t r : *rv) {
            if (r >= n) return fail(PQV_ERR_INVALID, range_text);
            member[r] = 1;
        }
        std::vector<uint32_t> new_id(n), h_old;
        h_old.reserve(n_pos);
        for (uint64_t r = 0; r < n; ++r) {
            new_id[r] = static_cast<uint32_t>(h_old.size());
            if (member[r]) h_old.push_back(static_cast<uint32_t>(r));
        }
        total = h_old.size();
        if (total != n_pos) return fail(PQV_ERR_INVALID, dup_text);
        idx->list_rows.resize(n_pos);
        for (uint64_t p = 0; p < n_pos; ++p) idx->list_rows[p] = new_id[(*rv)[p]];
        HIP_TRY(d_old_row.alloc(total * sizeof(uint32_t)));
        HIP_TRY(hipMemcpyAsync(d_old_row.p, h_old.data(), total * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));       // (h_old leaves scope)
    } else {
        std::shared_ptr<DevRows> old_dev;
        DevBuf d_up_ids, d_member, d_rowbits, d_rank, d_tmp, d_bad;
        const uint32_t *d_ids = nullptr;
        if (int rc = device_lists_of(index, corpus->device, n_pos, stream, old_dev, d_up_ids, &d_ids)) return rc;
        const uint64_t n_words = (n + 63) / 64;
        HIP_TRY(d_member.alloc(n));
        HIP_TRY(d_bad.alloc(sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(d_member.p, 0, n, stream));
        HIP_TRY(hipMemsetAsync(d_bad.p, 0, sizeof(uint32_t), stream));
        HIP_TRY(launch_member_bytes(d_ids, n_pos, n, d_member.as<uint8_t>(), d_bad.as<uint32_t>(), stream));
        HIP_TRY(d_rowbits.alloc((n_words + 1) * sizeof(uint64_t)));
        HIP_TRY(launch_mask_pack(d_member.as<uint8_t>(), n, d_rowbits.as<uint64_t>(), n_words, stream));
        HIP_TRY(d_rank.alloc((n_words + 1) * sizeof(uint64_t)));
        HIP_TRY(d_tmp.alloc((bit_rank_blocks(n) + 1) * sizeof(uint64_t)));
        HIP_TRY(launch_bit_rank(d_rowbits.as<uint64_t>(), n, false, d_rank.as<uint64_t>(), d_tmp.as<uint64_t>(), stream));
        uint32_t h_bad = 0;
        HIP_TRY(hipMemcpyAsync(&total, d_rank.as<uint64_t>() + n_words, sizeof total, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(&h_bad, d_bad.p, sizeof h_bad, hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        if (h_bad != 0) return fail(PQV_ERR_INVALID, range_text);
        if (total != n_pos) return fail(PQV_ERR_INVALID, dup_text);       // (the member count: a repeated row collapsed)
        HIP_TRY(d_old_row.alloc(total * sizeof(uint32_t)));
        HIP_TRY(d_new_rows.alloc(n_pos * sizeof(uint32_t)));
        HIP_TRY(launch_list_compact(nullptr, n, d_rowbits.as<uint64_t>(), false, d_rank.as<uint64_t>(), d_old_row.as<uint32_t>(), stream));
        HIP_TRY(launch_lists_remap(d_ids, n_pos, d_rowbits.as<uint64_t>(), n, d_rank.as<uint64_t>(), d_new_rows.as<uint32_t>(), stream));
        if (!keep_device_lists()) {
            idx->list_rows.resize(n_pos);
            HIP_TRY(hipMemcpyAsync(idx->list_rows.data(), d_new_rows.p, n_pos * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        }
        HIP_TRY(hipStreamSynchronize(stream));       // (the work buffers leave scope)
        if (keep_device_lists()) adopt_device_lists(idx.get(), d_new_rows, corpus->device, n_pos);
    }
    const double t1 = now_s();
    pqv_corpus *made = nullptr;
    if (int rc = pqv_corpus_create_impl(corpus->device, std::max(capacity_rows, total), dim, &made)) return rc;
    std::unique_ptr<pqv_corpus> dense(made);
    EventSet ev;
    DevBuf d_copy;
    const size_t row_bytes = static_cast<size_t>(total) * dim * sizeof(float);
    if (stats) {
        for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
        HIP_TRY(d_copy.alloc(row_bytes));
        HIP_TRY(hipEventRecord(ev.e[0], stream));
    }
    HIP_TRY(launch_rows_gather(corpus->d_rows, d_old_row.as<uint32_t>(), total, dim, dense->d_rows, stream));
    if (stats) {
        HIP_TRY(hipEventRecord(ev.e[1], stream));
        HIP_TRY(hipEventRecord(ev.e[2], stream));
        if (row_bytes) HIP_TRY(hipMemcpyAsync(d_copy.p, dense->d_rows, row_bytes, hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipEventRecord(ev.e[3], stream));
    }
    if (old_row && total) HIP_TRY(hipMemcpyAsync(old_row, d_old_row.p, total * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    dense->n = total;
    idx->set_row_bound(total);
    idx->permutation_of = total;                     // every new row is in exactly one list
    if (stats) {
        float ms_g = 0.0f, ms_copy = 0.0f;
        (void)hipEventElapsedTime(&ms_g, ev.e[0], ev.e[1]);
        (void)hipEventElapsedTime(&ms_copy, ev.e[2], ev.e[3]);
        std::fprintf(stderr, "pqv_index_compact: %llu of %llu rows stay: members + rank + lists %.3f ms, rows %.3f ms; gather kernel %.4f ms for "
                             "%.0f row bytes (%.1f GB/s written), device-to-device copy of the same bytes %.4f ms\n",
                     (unsigned long long)total, (unsigned long long)n, (t1 - t0) * 1e3, (now_s() - t1) * 1e3, ms_g, (double)row_bytes,
                     ms_g > 0.0f ? row_bytes / (ms_g * 1e6) : 0.0, ms_copy);
    }
    *corpus_out = dense.release();
    *index_out = idx.release();
    return PQV_OK;
}

}  // namespace

extern "C" int pqv_index_remove(const pqv_index *index, int device, const uint8_t *remove, uint64_t n_flags, pqv_index **out) {
    return guard([&] { return index_remove_impl(index, device, remove, nullptr, false, n_flags, nullptr, out); });
}
extern "C" int pqv_index_remove_device(const pqv_index *index, int device, const void *d_remove, uint64_t n_flags, void *hip_stream,
                                       pqv_index **out) {
    return guard([&] { return index_remove_impl(index, device, nullptr, d_remove, true, n_flags, hip_stream, out); });
}
extern "C" int pqv_index_remove_rows(const pqv_index *index, int device, const uint32_t *rows, uint64_t m, pqv_index **out) {
    return guard([&] { return index_remove_rows_impl(index, device, rows, m, out); });
}
extern "C" int pqv_index_compact(const pqv_index *index, const pqv_corpus *corpus, uint64_t capacity_rows, pqv_corpus **corpus_out,
                                 pqv_index **index_out, uint32_t *old_row) {
    return guard([&] { return index_compact_impl(index, corpus, capacity_rows, corpus_out, index_out, old_row); });
}

extern "C" int pqv_index_assign(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows,
                                uint32_t *cluster_out) {
    return guard([&] { return index_assign_impl(index, corpus, first_row, n_rows, cluster_out); });
}
extern "C" int pqv_index_append(const pqv_index *index, const pqv_corpus *corpus, uint64_t first_row, uint64_t n_rows,
                                pqv_index **out) {
    return guard([&] { return index_append_impl(index, corpus, first_row, n_rows, out); });
}

static int pqv_kpp_pick_impl(int device, const float *minima, uint32_t n, uint32_t workers, float draw, uint64_t *pick, float *total,
                             uint32_t *status) {
    using namespace pqv;
    if (!minima || !pick || !total || !status) return fail(PQV_ERR_INVALID, "minima, pick, total and status must not be NULL");
    if (n == 0 || n > 57344) return fail(PQV_ERR_INVALID, "n must be in [1, 57344]");
    if (int rc = use_device(device)) return rc;
    if (workers == 0) workers = host_workers();
    const uint64_t w = std::max<uint64_t>(1, std::min<uint64_t>(workers, n));          // index.rs:259-265
    const uint64_t chunk = (n + w - 1) / w, n_chunks = (n + chunk - 1) / chunk;
    if (n_chunks > 1024) return fail(PQV_ERR_INVALID, "more than 1024 worker chunks");
    KppScratch scratch;                                // two pick slots (round 1 writes the second), four draws, the minima behind them
    if (int rc = scratch.init(2, 4, n_chunks, n, nullptr)) return rc;
    const float u2[2] = {0.0f, draw};
    HIP_TRY(hipMemcpy(scratch.draws, u2, sizeof u2, hipMemcpyHostToDevice));
    HIP_TRY(hipMemcpy(scratch.minima, minima, static_cast<size_t>(n) * 4, hipMemcpyHostToDevice));
    KppPickArgs pa = scratch.pa;
    pa.md = scratch.minima; pa.n = n; pa.chunk = static_cast<uint32_t>(chunk); pa.round = 1;
    DevBuf d_stamps;
    const char *want_stamps = std::getenv("PQV_KPP_STAMPS");
    if (want_stamps && *want_stamps == '1') {
        HIP_TRY(d_stamps.alloc(48 * 8));
        HIP_TRY(hipMemset(d_stamps.p, 0, 48 * 8));
        pa.stamps = d_stamps.as<unsigned long long>();
    }
    HIP_TRY(launch_kpp_pick(pa, nullptr));
    HIP_TRY(hipDeviceSynchronize());
    if (pa.stamps) {
        unsigned long long h[48];
        HIP_TRY(hipMemcpy(h, d_stamps.p, sizeof h, hipMemcpyDeviceToHost));
        unsigned long long t0 = ~0ull;
        for (int i = 0; i < 40; ++i) if (h[i] && h[i] < t0) t0 = h[i];
        std::fprintf(stderr, "[pqv] kpp stamps (us after the first; chain block 0-7: start, loaded, summaries there, pairs read, chain done, total, found, picked;"
                             " last summary block 8-12: start, sum out, prefix in, pairs, flag out; chunk block 0 16-17; end of wave w's turn 20+w):");
        for (int i = 0; i < 40; ++i) if (h[i]) std::fprintf(stderr, " %d:%.2f", i, (h[i] - t0) * 0.01);
        std::fprintf(stderr, "\n");
    }
    uint32_t h_state[4];
    unsigned long long h_pick[2];
    HIP_TRY(hipMemcpy(h_state, pa.state, sizeof h_state, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(h_pick, pa.picks, sizeof h_pick, hipMemcpyDeviceToHost));
    *status = h_state[0] ? h_state[2] : 0;
    std::memcpy(total, &h_state[3], 4);
    if (!h_state[0]) *pick = h_pick[1];
    return PQV_OK;
}
extern "C" int pqv_kpp_pick(int device, const float *minima, uint32_t n, uint32_t workers, float draw, uint64_t *pick, float *total,
                            uint32_t *status) {
    return guard([&] { return pqv_kpp_pick_impl(device, minima, n, workers, draw, pick, total, status); });
}

extern "C" int pqv_index_build_stats(double *out, uint32_t n) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    for (uint32_t i = 0; i < n; ++i) out[i] = i < BS_COUNT ? g_build_stats[i] : 0.0;
    return PQV_OK;
}

static int pqv_index_build_host_impl(int device, const float *data, uint64_t data_len, uint32_t dim,
                                    uint32_t n_clusters, uint32_t max_iters, uint64_t seed,
                                    uint32_t workers, pqv_index **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");     // mod.rs:59
    if (data_len % dim != 0)
        return fail(PQV_ERR_INVALID, "Embedding data length must be a multiple of dimension"); // mod.rs:86
    if (max_iters == 0) return fail(PQV_ERR_INVALID, "max_iters must be > 0");
    const uint64_t n = data_len / dim;
    if (n == 0) return fail(PQV_ERR_INVALID, "Cannot build IVF index with zero vectors");
    pqv_corpus *c = nullptr;
    if (int rc = pqv_corpus_upload(device, data, n, dim, &c)) return rc;
    const int rc = build_index_impl(c, n_clusters, max_iters, seed, workers, out);
    pqv_corpus_free(c);
    return rc;
}
extern "C" int pqv_index_build_host(int device, const float *data, uint64_t data_len, uint32_t dim,
                                    uint32_t n_clusters, uint32_t max_iters, uint64_t seed,
                                    uint32_t workers, pqv_index **out) {
    return guard([&] { return pqv_index_build_host_impl(device, data, data_len, dim, n_clusters, max_iters, seed, workers, out); });
}

static int pqv_kmeans_impl(const pqv_corpus *sample, uint32_t k, uint32_t max_iters, uint64_t seed,
                          uint32_t workers, float *centroids, uint32_t *assignments,
                          uint32_t *iters_run) {
    if (!sample || !centroids) return fail(PQV_ERR_INVALID, "sample/centroids must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "Cluster count must be > 0");
    if (sample->n == 0 || k > sample->n) return fail(PQV_ERR_INVALID, "n_clusters cannot exceed number of vectors");
    if (!sample->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    if (int rc = use_device(sample->device)) return rc;
    DevBuf d_centroids;
    HIP_TRY(d_centroids.alloc(static_cast<size_t>(k) * sample->dim * sizeof(float)));
    std::vector<uint32_t> assign;
    if (int rc = kmeans_device(sample->d_rows, sample->n, sample->dim, k, max_iters, seed, workers,
                               sample->stream, d_centroids.as<float>(), &assign, iters_run))
        return rc;
    HIP_TRY(hipMemcpy(centroids, d_centroids.p, static_cast<size_t>(k) * sample->dim * sizeof(float),
                      hipMemcpyDeviceToHost));
    if (assignments) std::memcpy(assignments, assign.data(), assign.size() * sizeof(uint32_t));
    return PQV_OK;
}
extern "C" int pqv_kmeans(const pqv_corpus *sample, uint32_t k, uint32_t max_iters, uint64_t seed,
                          uint32_t workers, float *centroids, uint32_t *assignments,
                          uint32_t *iters_run) {
    return guard([&] { return pqv_kmeans_impl(sample, k, max_iters, seed, workers, centroids, assignments, iters_run); });
}

// ---------------------------------------------------------------------------------------
// searcher
// ---------------------------------------------------------------------------------------
namespace {

void opts_from_env(pqv_searcher::Opts &o) {
    auto num = [](const char *name, long long dflt) { const char *e = std::getenv(name); return e && *e ? std::strtoll(e, nullptr, 10) : dflt; };
    if (const char *m = std::getenv("PQV_RERANK_MODE")) o.rerank_mode = !std::strcmp(m, "stream") ? 1 : !std::strcmp(m, "tile") ? 2 : 0;
    o.tile_filter = static_cast<int>(std::min<long long>(2, std::max<long long>(0, num("PQV_TILE_FILTER", o.tile_filter))));
    o.filter_variant = static_cast<int>(num("PQV_FILTER_VARIANT", o.filter_variant));
    o.cand_cap = static_cast<uint32_t>(std::max<long long>(0, num("PQV_CAND_CAP", o.cand_cap)));
    o.screen_f16 = num("PQV_SCREEN_F16", o.screen_f16) != 0;
    o.screen_i8 = static_cast<int>(num("PQV_SCREEN_I8", o.screen_i8));
    o.seed_rows = static_cast<uint32_t>(num("PQV_SEED_ROWS", o.seed_rows));
    o.wide_rows = static_cast<uint32_t>(num("PQV_WIDE_ROWS", o.wide_rows));
    o.tile_rows = static_cast<uint32_t>(num("PQV_TILE_ROWS", o.tile_rows));
    o.running_thr = num("PQV_RUNNING_THR", o.running_thr) != 0;
    o.defer = static_cast<int>(num("PQV_DEFER", o.defer));
    o.quad_xcd = static_cast<int>(num("PQV_QUAD_XCD", o.quad_xcd));
    o.wide_waves = static_cast<int>(num("PQV_WIDE_WAVES", o.wide_waves));
    o.item_grid = static_cast<int>(num("PQV_ITEM_GRID", o.item_grid));
    o.chunk_major = static_cast<int>(num("PQV_CHUNK_MAJOR", o.chunk_major));
    o.seed_refine = static_cast<int>(num("PQV_SEED_REFINE", o.seed_refine));
    o.single_bucket = static_cast<int>(num("PQV_SINGLE_BUCKET", o.single_bucket));
    o.probe_rows = static_cast<int>(num("PQV_PROBE_ROWS", o.probe_rows));
    o.probe_screen = static_cast<int>(num("PQV_PROBE_SCREEN", o.probe_screen));
    o.quad_width = static_cast<uint32_t>(num("PQV_QUAD_WIDTH", o.quad_width));
    o.min_blocks = static_cast<uint32_t>(num("PQV_MIN_BLOCKS", o.min_blocks));
    o.wide_quads = static_cast<int>(num("PQV_WIDE_QUADS", o.wide_quads));
    o.fork_wide = static_cast<int>(num("PQV_FORK_WIDE", o.fork_wide));
    o.drain_min = static_cast<int>(num("PQV_DRAIN_MIN", o.drain_min));
    o.pf96 = static_cast<int>(num("PQV_PF96", o.pf96));
    o.static_dim = num("PQV_STATIC_DIM", o.static_dim) != 0 ? 1 : 0;
    o.xcd_items = static_cast<int>(num("PQV_XCD_ITEMS", o.xcd_items));
    o.wide_quad_rows = static_cast<uint32_t>(num("PQV_WIDE_QUAD_ROWS", o.wide_quad_rows));
    o.list_once = static_cast<int>(num("PQV_LIST_ONCE", o.list_once));
    o.partition_blocks = static_cast<uint32_t>(std::max<long long>(0, num("PQV_PARTITION_BLOCKS", o.partition_blocks)));
    o.partition_range_bytes = static_cast<uint64_t>(std::max<long long>(0, num("PQV_PARTITION_RANGE_BYTES", static_cast<long long>(o.partition_range_bytes))));
    o.pair_prune = static_cast<int>(num("PQV_PAIR_PRUNE", o.pair_prune));
    o.i8_form = static_cast<int>(num("PQV_I8_FORM", o.i8_form));
}

// Cache policy of the wide-quad instance's row stream (kernels_screen.hip, launch_filter_s): nt unless a recent batch had more than a
// quarter of its wide work items in lists of several quads (those share their rows through the caches).  A hint only: it
// is read without synchronisation and never changes a result; before the first batch has reported: nt.
bool wide_rows_nt(const pqv_searcher *s) {
    if (!s->h_wide_stats.p) return true;
    const volatile uint32_t *h = s->h_wide_stats.as<uint32_t>();
    const uint32_t total = h[0], lone = h[1];
    return total == 0 || static_cast<uint64_t>(lone) * 4 >= static_cast<uint64_t>(total) * 3;
}

// Wide-quad instance or regular quads only?  A list probed by 97..160 queries is read ONCE by a wide quad (32-row tiles, one
// 8-wave block per CU, 4.7 TB/s) instead of twice by two regular quads -- uniform C3: 585 against 549 k q/s.  A list probed by
// HUNDREDS of queries (clustered queries) is read by several quads either way; the regular ones then share its rows through one
// XCD's L2 (PairSortArgs::xcd_items) at the regular instance's rate -- mixture: kernels 2.13 against 2.34 ms.  The previous
// batch's shape decides (pair_scan_kernel -> pinned memory; an unsynchronised hint that never changes a result): regular only
// when more than half of the rows in lists of > 96 pairs sit in lists of > 160 (and such lists hold >= 1 / 32 of the corpus).
bool prefer_regular(const pqv_searcher *s) {
    if (!s->h_wide_stats.p) return false;
    const volatile uint32_t *h = s->h_wide_stats.as<uint32_t>();
    const uint32_t multi = h[2], pop = h[3];
    // (... and those popular lists are a real part of the corpus -- 1 / 32 of its rows: a uniform batch on short lists has a
    //  handful of them, and their split says nothing about the query load)
    return static_cast<uint64_t>(pop) * 32 >= s->n && static_cast<uint64_t>(multi) * 2 > pop;
}

// the wide screened kernels need IVF-ordered rows of a multiple of 64 dims
bool wide_path_possible(const pqv_searcher *s) { return (s->sdim % 64) == 0 && (!s->d_row_of || s->images_only) && s->n > 0; }

// Operand form of the screen for this searcher (pqv::ScreenOp numbering: 0 f32, 1 f16, 2 int8)
// int8 images halve the bytes per streamed row but widen the bound (residual norms): where lists are short and k is
// large the extra exact evaluations cost more than the stream saves -- measured on the reference's bench shape (1 M x
// 1024, 1000-row lists): K = 100 int8 2.93 against f16 2.31 ms per step, K = 10 equal; C3 (9766-row lists) K = 10
// 2.44 against 3.85, K = 100 4.21 against 5.10; 1 M x 768 (976-row lists) K = 10 1.07 against 1.16.
// squared norms of the rows for the f32 / f16 MFMA screens (indexed by storage row; by list position in the images-only layout) and, in
// the same pass, the corpus maximum -> power-of-two scale that maps it below 2^14 (f16 operand copy).  Once per searcher.
int ensure_row_norms(const pqv_searcher *s, hipStream_t stream) {
    std::lock_guard<std::mutex> lock(s->norms_mu);
    if (s->norms_done) return PQV_OK;
    DevBuf d_max;
    HIP_TRY(d_max.alloc(sizeof(uint32_t)));
    HIP_TRY(hipMemsetAsync(d_max.p, 0, sizeof(uint32_t), stream));
    HIP_TRY(s->d_row_norm2.alloc(std::max<uint64_t>(1, s->n_storage) * sizeof(float)));
    HIP_TRY(pqv::launch_row_norms_max(s->d_mat, s->images_only ? s->d_row_of : nullptr, s->n_storage, s->sdim, s->d_row_norm2.as<float>(),
                                      d_max.as<uint32_t>(), stream));
    uint32_t bits = 0;
    HIP_TRY(hipMemcpyAsync(&bits, d_max.p, sizeof bits, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    float m;
    std::memcpy(&m, &bits, sizeof m);
    if (bits < 0x7F800000u) {
        int e = 0;
        if (m > 0.0f) (void)std::frexp(m, &e);           // m = f * 2^e, f in [0.5, 1)  =>  m < 2^e
        const int se = m > 0.0f ? 14 - e : 0;            // scale = 2^se: m * scale < 2^14
        if (se >= -60 && se <= 60) { s->f16_ok = true; s->f16_scale = std::ldexp(1.0f, se); }
    }
    s->norms_done = true;
    return PQV_OK;
}

constexpr int kNotFinite = -9001;      // ensure_blocked_copy(op 2) at creation: the rows are not all finite and moderate (the caller falls back)

int screen_op(const pqv_searcher *s, uint32_t k = 1) {
    const uint64_t mean_len = s->n / std::max<uint32_t>(1, s->n_clusters);
    const bool i8_pays = !(k > 32 && mean_len < 4096) || s->opt.screen_i8 > 1;
    if (s->opt.screen_i8 && i8_pays && s->i8_ok && (s->sdim % 256) == 0 && s->sdim >= 256 && static_cast<uint64_t>(64) * s->sdim <= 147456) return 2;
    if (!s->norms_done && ensure_row_norms(s, s->stream) != PQV_OK) return 0;      // (f16_ok is known only after that pass)
    if (s->opt.screen_f16 && s->f16_ok && (s->sdim % 128) == 0 && s->sdim <= 1024) return 1;
    return 0;
}

// One-off: the blocked MFMA-operand copy of the lists (a second copy of the corpus in HBM: f16 half its size,
// int8 a quarter)
int ensure_blocked_copy(const pqv_searcher *s, int op, hipStream_t stream) {
    using namespace pqv;
    DevBuf &blk = s->d_mat_blk_op[op];
    if (blk.p) return PQV_OK;
    // A copy counts as built only once its LAST step has succeeded: any failure on the way (an allocation, a launch, a
    // synchronisation) releases it, so that the next call rebuilds instead of screening against half-written images, row
    // terms or list scales (the bound would no longer hold and true neighbours could be pruned silently).
    struct Undo {
        const pqv_searcher *s; DevBuf &blk; int op; bool done = false;
        ~Undo() {
            if (done) return;
            (void)hipDeviceSynchronize();       // nothing still in flight may write into what is released
            blk.release();
            if (op == 2) {
                s->d_row_n2i.release(); s->d_row_res.release(); s->d_center.release(); s->d_list_scale.release();
                s->d_list_half.release(); s->d_list_radius.release(); s->i8_residual = true;
            }
        }
    } undo{s, blk, op};
    const uint32_t kc = s->n_clusters;
    std::vector<uint64_t> boff(static_cast<size_t>(kc) + 1, 0);
    for (uint32_t c = 0; c < kc; ++c) boff[c + 1] = boff[c] + (s->h_list_off[c + 1] - s->h_list_off[c] + 15) / 16;
    if (!s->d_blk_off.p) {
        HIP_TRY(s->d_blk_off.alloc(boff.size() * sizeof(uint64_t)));
        const hipError_t ce = hipMemcpy(s->d_blk_off.p, boff.data(), boff.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
        if (ce != hipSuccess) { s->d_blk_off.release(); HIP_TRY(ce); }
    }
    const uint64_t tiles = std::max<uint64_t>(1, boff[kc]);
    if (op != 2) { if (int rc = ensure_row_norms(s, stream)) return rc; }
    if (op == 2) {
        HIP_TRY(blk.alloc(tiles * 16 * s->sdim));
        HIP_TRY(s->d_row_n2i.ensure(std::max<uint64_t>(1, s->n) * sizeof(int)));
        HIP_TRY(s->d_row_res.ensure(std::max<uint64_t>(1, s->n) * sizeof(float)));
        // per-list centre (mid-range per dimension), half range, scale; then the images, row terms and list radii
        const size_t cd = static_cast<size_t>(std::max<uint32_t>(1, kc)) * s->sdim;
        DevBuf d_mm;
        HIP_TRY(d_mm.alloc(2 * cd * sizeof(uint32_t)));
        uint32_t *kmin = d_mm.as<uint32_t>(), *kmax = kmin + cd;
        HIP_TRY(hipMemsetAsync(kmin, 0xFF, cd * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(kmax, 0, cd * sizeof(uint32_t), stream));
        HIP_TRY(s->d_center.alloc(cd * sizeof(float)));
        HIP_TRY(s->d_list_scale.alloc(std::max<uint32_t>(1, kc) * sizeof(float)));
        HIP_TRY(s->d_list_half.alloc(std::max<uint32_t>(1, kc) * sizeof(float)));
        HIP_TRY(s->d_list_radius.alloc(std::max<uint32_t>(1, kc) * sizeof(float)));
        HIP_TRY(launch_list_minmax(s->d_mat, s->d_list_off.as<uint64_t>(), kc, s->max_list_len, s->sdim, kmin, kmax, stream, s->d_row_of));
        HIP_TRY(launch_list_center(kmin, kmax, kc, s->sdim, s->d_list_off.as<uint64_t>(), s->d_center.as<float>(), s->d_list_half.as<float>(),
                                   s->d_list_scale.as<float>(), s->d_list_radius.as<float>(), stream));
        {   // residual or one-centre form: compare the lists' scales with the scale ONE centre for the whole corpus would get
            DevBuf d_g;
            HIP_TRY(d_g.alloc((static_cast<size_t>(s->sdim) + 2) * sizeof(float)));
            float *g_center = d_g.as<float>(), *g_hs = g_center + s->sdim;
            HIP_TRY(launch_global_center(kmin, kmax, kc, s->sdim, s->d_list_off.as<uint64_t>(), g_center, g_hs, stream));
            std::vector<float> h_scale(std::max<uint32_t>(1, kc));
            float h_g[2] = {0.0f, 1.0f};
            std::vector<float> h_gc(s->norms_done ? 0 : s->sdim);
            HIP_TRY(hipMemcpyAsync(h_scale.data(), s->d_list_scale.p, static_cast<size_t>(kc) * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipMemcpyAsync(h_g, g_hs, sizeof h_g, hipMemcpyDeviceToHost, stream));
            if (!h_gc.empty()) HIP_TRY(hipMemcpyAsync(h_gc.data(), g_center, h_gc.size() * sizeof(float), hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (!s->norms_done) {
                // No pass over the rows' norms has vouched for the data (creation builds this copy first): the per-dimension extremes
                // do -- every |x_d| <= |mid-range_d| + half range =: m, at most twice the true maximum.  ensure_row_norms' rule is
                // "finite, and 2^-46 <= max |x_d| < 2^74"; anything within a factor of two of those ends, an infinity or a NaN (it
                // shows in the extremes) sends the caller to that pass, which decides exactly.
                float m = 0.0f;
                bool fin = h_g[0] == h_g[0] && h_g[0] < 1.0e30f;
                for (float c : h_gc) { fin = fin && c == c; m = std::max(m, std::fabs(c)); }
                m += h_g[0];
                if (verbose()) std::fprintf(stderr, "[pqv] int8 copy first: half range %.4g, largest |value| <= %.4g, finite %d\n", h_g[0], m, fin ? 1 : 0);
                if (!fin || !(m < 9.0e21f) || !(m > 3.0e-14f)) { s->i8_ok = false; return kNotFinite; }
            }
            // row-weighted median of the list scales (an empty or one-point list says nothing about the data)
            std::vector<std::pair<float, uint64_t>> sc;
            uint64_t rows_total = 0;
            for (uint32_t c = 0; c < kc; ++c) {
                const uint64_t len = s->h_list_off[c + 1] - s->h_list_off[c];
                if (len >= 2) { sc.emplace_back(h_scale[c], len); rows_total += len; }
            }
            std::sort(sc.begin(), sc.end());
            float med = h_g[1];
            uint64_t acc = 0;
            for (const auto &e : sc) { acc += e.second; if (2 * acc >= rows_total) { med = e.first; break; } }
            const int form = s->opt.i8_form;
            s->i8_residual = form == 2 || (form != 1 && med >= 1.3f * h_g[1]);
            if (!s->i8_residual)
                HIP_TRY(launch_broadcast_center(g_center, g_hs, kc, s->sdim, s->d_center.as<float>(), s->d_list_half.as<float>(),
                                                s->d_list_scale.as<float>(), stream));
            if (verbose()) std::fprintf(stderr, "[pqv] int8 images: median list scale %.4g, one-centre scale %.4g -> %s form\n", med, h_g[1],
                                        s->i8_residual ? "per-list residual" : "one-centre");
            HIP_TRY(hipStreamSynchronize(stream));      // d_g is released at scope exit
        }
        HIP_TRY(launch_block_rows_i8(s->d_mat, s->d_list_off.as<uint64_t>(), s->d_blk_off.as<uint64_t>(), kc,
                                     (s->max_list_len + 15) / 16, s->sdim, s->d_center.as<float>(), s->d_list_scale.as<float>(),
                                     s->d_list_half.as<float>(), s->d_list_radius.as<float>(), blk.p, s->d_row_n2i.as<int>(),
                                     s->d_row_res.as<float>(), stream, s->d_row_of));
        HIP_TRY(hipStreamSynchronize(stream));      // d_mm is released at scope exit
    } else if (op == 1) {
        HIP_TRY(blk.alloc(tiles * 16 * s->sdim * 2));
        HIP_TRY(launch_block_rows_f16(s->d_mat, s->d_list_off.as<uint64_t>(), s->d_blk_off.as<uint64_t>(), kc,
                                      (s->max_list_len + 15) / 16, s->sdim, s->f16_scale, blk.p, stream, s->d_row_of));
    } else {
        HIP_TRY(blk.alloc(tiles * 16 * s->sdim * sizeof(float)));
        HIP_TRY(launch_block_rows(s->d_mat, s->d_list_off.as<uint64_t>(), s->d_blk_off.as<uint64_t>(), kc,
                                  (s->max_list_len + 15) / 16, s->sdim, blk.p, stream, s->d_row_of));
    }
    HIP_TRY(hipStreamSynchronize(stream));      // one-off; calls on other streams may follow at once
    undo.done = true;
    return PQV_OK;
}

// The screened probe's centroid side, made once per searcher: mu = the centroid mean (any fixed vector serves the bound; the mean
// shrinks |q - mu| |c - mu|, which scales its slack), f16 images of (c - mu) at ONE scale 2^8 / max |c - mu|, |c - mu|^2, and the
// constants of probe_bound (kernels_probe_screen.hip; derivation in DESIGN 5.1), in units of 2^-24 = u and 2^-11 = h:
//   e1  per |a||b|: 2 h' + h'^2 (h' = h + u + h u: both images rounded to f16 after an f32 product), the contraction's f32
//       accumulation in any order (2.02 dim_p u), the query image's subnormal components, the roundings of the estimate
//   e2s per |a|: sqrt(dim) 2^-25 / cscale -- components of a centroid image below 2^-14 carry an ABSOLUTE rounding error
//   kS  per |a|^2 + |b|^2: the norms' summation (center_normalize_f16_sum_depth), the roundings of q - mu and c - mu, of the sum
//   cm  = (dim / 4 + 8) u: the reference chain rounds each term six times and the running sum once per group, all terms >= 0
// ps.ok stays false -- the plan keeps probe_rows_kernel -- for a table with a non-finite norm or a scale f32 cannot hold.
hipError_t probe_screen_images(pqv_searcher *s) {
    using namespace pqv;
    const uint32_t kc = s->n_clusters, dim = s->dim, dim_p = (dim + 63) / 64 * 64;
    s->ps.tried = true;
#define PS_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return _e; } while (0)
    PS_TRY(s->d_ps_mu.alloc(static_cast<size_t>(dim) * sizeof(float)));
    PS_TRY(s->d_ps_c16.alloc(static_cast<size_t>(s->kc_pad) * dim_p * sizeof(uint16_t)));
    PS_TRY(s->d_ps_cn2.alloc(static_cast<size_t>(s->kc_pad) * sizeof(float)));
    const float *d_c = s->d_centroids.as<float>();
    PS_TRY(launch_col_mean(d_c, kc, dim, s->d_ps_mu.as<float>(), s->stream));
    // the norms first (the images of this pass are overwritten below), then the images at the scale the norms give
    PS_TRY(launch_center_normalize_f16(d_c, s->d_ps_mu.as<float>(), kc, s->kc_pad, dim, dim_p, s->d_ps_cn2.as<float>(), s->d_ps_c16.p, s->stream));
    std::vector<float> h_cn2(kc);
    PS_TRY(hipMemcpyAsync(h_cn2.data(), s->d_ps_cn2.p, static_cast<size_t>(kc) * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    PS_TRY(hipStreamSynchronize(s->stream));
    double mx = 0.0;
    for (float v : h_cn2) { if (!(v <= 3.0e38f)) return hipSuccess; mx = std::max<double>(mx, v); }
    const float cscale = mx > 0.0 ? static_cast<float>(256.0 / (std::sqrt(mx) * 1.000001)) : 1.0f;
    const float inv_cs = static_cast<float>(1.000001 / static_cast<double>(cscale));
    if (!(cscale > 0.0f && cscale < 3.0e38f && inv_cs > 0.0f && inv_cs < 3.0e38f)) return hipSuccess;
    PS_TRY(launch_center_normalize_f16(d_c, s->d_ps_mu.as<float>(), kc, s->kc_pad, dim, dim_p, s->d_ps_cn2.as<float>(), s->d_ps_c16.p, s->stream, cscale));
#undef PS_TRY
    const double u = 5.9604644775390625e-08, h = 4.8828125e-04, hp = h + u + h * u;
    const double sub = std::sqrt(static_cast<double>(dim)) * 2.98023223876953125e-08;
    const double g = (center_normalize_f16_sum_depth(dim) + 2) * u * 1.01;
    const double cm = (dim / 4 + 8) * u;
    auto up = [](double v) { return std::nextafter(static_cast<float>(v), INFINITY); };
    pqv_searcher::ProbeScreen &ps = s->ps;
    ps.dim_p = dim_p; ps.inv_cs = inv_cs;
    ps.fn = up((1.0 + g) * 1.000001);
    ps.e1 = up((2.0 * hp + hp * hp + 1.01 * 2.02 * dim_p * u + 1.01 * sub / 256.0 + 2.0e-6) * 1.001);
    ps.e2s = up(static_cast<double>(inv_cs) * sub * 1.02);
    ps.kS = up(1.01 * g + 16.0 * u);
    ps.lo_f = std::nextafter(static_cast<float>(1.0 - cm - 1.0e-6), 0.0f);
    ps.hi_f = up(1.0 + cm + 1.0e-6);
    ps.ok = ps.e2s < 3.0e38f;
    if (const char *e = std::getenv("PQV_PROBE_SCREEN_STATS"); e && *e && *e != '0') {
        if (s->d_ps_stats.alloc(3 * sizeof(unsigned long long)) == hipSuccess) (void)hipMemsetAsync(s->d_ps_stats.p, 0, 3 * sizeof(unsigned long long), s->stream);
    }
    return hipSuccess;
}

}  // namespace

static int pqv_searcher_create_impl(const pqv_index *index, pqv_corpus *corpus, uint32_t flags,
                                   pqv_searcher **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    const auto t_enter = std::chrono::steady_clock::now();
    if (!index || !corpus) return fail(PQV_ERR_INVALID, "index/corpus must not be NULL");
    if (index->dim != corpus->dim)
        return fail(PQV_ERR_INVALID, "index dimension " + std::to_string(index->dim) +
                                         " does not match corpus dimension " + std::to_string(corpus->dim));
    if (index->permutation_of != 0 ? index->permutation_of != corpus->n : false)
        return fail(PQV_ERR_INVALID, "index row id out of range for this corpus");
    // (a build's lists are a permutation of the corpus' rows; anything else is checked: by the row bound where the index knows one
    //  that fits -- an appended or a removed index, whose lists may still be on the device -- else row by row)
    uint64_t known_bound = 0;
    if (index->permutation_of == 0 && !(index->known_row_bound(&known_bound) && known_bound <= corpus->n)) {
        const std::vector<uint32_t> *rv = index->rows->get();
        if (!rv) return PQV_ERR_HIP;
        for (uint32_t r : *rv)
            if (r >= corpus->n) return fail(PQV_ERR_INVALID, "index row id out of range for this corpus");
    }
    if (!corpus->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    if (int rc = use_device(corpus->device)) return rc;
    pqv_searcher *s = new (std::nothrow) pqv_searcher();
    if (!s) return fail(PQV_ERR_OOM, "host allocation failed");
    { static std::atomic<uint64_t> next_uid{1}; s->uid = next_uid.fetch_add(1, std::memory_order_relaxed); }
    s->device = corpus->device; s->dim = index->dim; s->sdim = index->dim; s->n_clusters = index->n_clusters;
    if (!(flags & PQV_LAYOUT_ROW_ORDER) && (s->dim % 4) == 0 && (s->dim % 64) != 0) {
        // zero-padded storage: the cheapest tiling whose padding stays within a third of the row -- int8 images (a multiple
        // of 256 dims), else f16 (128), else f32 (64); rows of fewer than 48 dims stay as they are (exact kernels)
        auto up = [&](uint32_t m) { return (s->dim + m - 1) / m * m; };
        const uint64_t lim = static_cast<uint64_t>(s->dim) * 4 / 3;
        if (s->dim >= 192 && up(256) <= lim) s->sdim = up(256);
        else if (up(128) <= lim) s->sdim = up(128);
        else if (up(64) <= lim) s->sdim = up(64);
    }
    s->n = index->n_rows(); s->corpus = corpus;
    s->h_list_off = index->list_off; s->h_rows = index->rows;
    for (uint32_t c = 0; c < index->n_clusters; ++c)
        s->max_list_len = std::max<uint64_t>(s->max_list_len, index->list_off[c + 1] - index->list_off[c]);
    auto cleanup = [&](int code, const std::string &msg) { delete s; return fail(code, msg); };
#define S_TRY(expr)                                                                       \
    do {                                                                                  \
        hipError_t _e = (expr);                                                           \
        if (_e != hipSuccess)                                                             \
            return cleanup(_e == hipErrorOutOfMemory ? PQV_ERR_OOM : PQV_ERR_HIP,         \
                           std::string(#expr) + ": " + hipGetErrorString(_e));           \
    } while (0)
    opts_from_env(s->opt);
    // PQV_CREATE_STATS=1: wall time of the phases below on stderr (diagnostic; synchronises the stream at every mark)
    const bool create_stats = std::getenv("PQV_CREATE_STATS") != nullptr;
    auto t_last = t_enter;
    auto mark = [&](const char *what) {
        if (!create_stats) return;
        if (s->stream) (void)hipStreamSynchronize(s->stream);
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "pqv_searcher_create: %-28s %8.2f ms\n", what, std::chrono::duration<double, std::milli>(now - t_last).count());
        t_last = now;
    };
    mark("validation + host copies");
    S_TRY(pool_get(s->device, &s->stream));
    mark("stream");
    S_TRY(s->d_centroids.alloc(index->centroids.size() * sizeof(float)));
    S_TRY(s->d_list_off.alloc(index->list_off.size() * sizeof(uint64_t)));
    S_TRY(s->d_ids.alloc(std::max<size_t>(1, s->n) * sizeof(uint32_t)));
    mark("allocations");
    S_TRY(hipMemcpyAsync(s->d_centroids.p, index->centroids.data(), index->centroids.size() * sizeof(float),
                         hipMemcpyHostToDevice, s->stream));
    S_TRY(hipMemcpyAsync(s->d_list_off.p, index->list_off.data(), index->list_off.size() * sizeof(uint64_t),
                         hipMemcpyHostToDevice, s->stream));
    if ((s->dim % 4) == 0 && s->n_clusters) {
        s->kc_pad = (s->n_clusters + 255) / 256 * 256;
        S_TRY(s->d_cent_t.alloc(static_cast<size_t>(s->kc_pad) * s->dim * sizeof(float)));
        S_TRY(pqv::launch_transpose_rows4(s->d_centroids.as<float>(), s->n_clusters, s->kc_pad, s->dim, s->d_cent_t.p, s->stream));
        if (s->opt.probe_screen) {
            if (hipError_t e = probe_screen_images(s)) S_TRY(e);
        }
    }
    mark("centroid tables");
    if (s->n) {
        const DevRows *dr = index->rows->dev.get();
        if (dr && dr->p && dr->device == s->device && dr->n == s->n) {      // the build's device copy
            S_TRY(hipMemcpyAsync(s->d_ids.p, dr->p, s->n * sizeof(uint32_t), hipMemcpyDeviceToDevice, s->stream));
        } else {
            const std::vector<uint32_t> *rv = index->rows->get();
            if (!rv) { delete s; return PQV_ERR_HIP; }
            S_TRY(hipMemcpyAsync(s->d_ids.p, rv->data(), s->n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
        }
    }
    mark("tables + ids upload");
    // images-only IVF layout: where the wide screened path will serve this searcher (rows of a multiple of 64 dims, lists of
    // >= 192 rows on average) and the caller's matrix stays (no PQV_RELEASE_ROW_ORDER); PQV_IVF_COPY=1 keeps the second copy (A/B)
    {
        const char *e = std::getenv("PQV_IVF_COPY");
        const bool want_copy = e && *e && *e != '0';
        s->images_only = !(flags & PQV_LAYOUT_ROW_ORDER) && !((flags & PQV_RELEASE_ROW_ORDER) && corpus->owned) && !want_copy && s->sdim == s->dim &&
                         (s->dim % 64) == 0 && s->n > 0 && s->n / std::max<uint32_t>(1, s->n_clusters) >= 192;
    }
    if ((flags & PQV_LAYOUT_ROW_ORDER) || s->images_only) {
        s->d_mat = corpus->d_rows;
        s->d_row_of = s->d_ids.as<uint32_t>();
        s->d_final_ids = nullptr;
    } else {
        S_TRY(s->d_mat_ivf.alloc(std::max<size_t>(1, s->n) * s->sdim * sizeof(float)));
        mark("allocate the IVF-ordered copy");
        if (s->sdim != s->dim)
            S_TRY(pqv::launch_pad_rows(corpus->d_rows, s->d_ids.as<uint32_t>(), s->n, s->dim, s->sdim, s->d_mat_ivf.as<float>(), s->stream));
        else
        S_TRY(pqv::launch_gather_rows(corpus->d_rows, s->d_ids.as<uint32_t>(), nullptr, s->n, s->dim,
                                      s->d_mat_ivf.as<float>(), s->stream));
        s->d_mat = s->d_mat_ivf.as<float>();
        s->d_row_of = nullptr;
        s->d_final_ids = s->d_ids.as<uint32_t>();
    }
    mark("gather rows into list order");
#ifdef PQV_PROFILE_PHASES
    S_TRY(s->d_stats.alloc((8 + 8 * 65536) * sizeof(unsigned long long)));
    S_TRY(hipMemsetAsync(s->d_stats.p, 0, (8 + 8 * 65536) * sizeof(unsigned long long), s->stream));
#else
    S_TRY(s->d_stats.alloc((8 + 16 * pqv::STATS_SLOTS) * sizeof(unsigned long long)));
    S_TRY(hipMemsetAsync(s->d_stats.p, 0, (8 + 16 * pqv::STATS_SLOTS) * sizeof(unsigned long long), s->stream));
#endif
    s->n_storage = (flags & PQV_LAYOUT_ROW_ORDER) ? corpus->n : s->n;
    // The blocked MFMA-operand copy of the lists is built here, not inside the first query, whenever the wide screened path can apply
    // to this searcher (ensure_blocked_copy rebuilds it if an option changes its form).  int8 form: rows of a multiple of 256 dims,
    // IVF-ordered rows, finite data.  Where that copy is built right away, ITS first pass (the per-dimension extremes) vouches for the
    // data and the rows' norms -- 5.5 ms of C3's creation, never read by the int8 screen -- wait for a call that needs them.
    const bool build_now = wide_path_possible(s) && s->n / std::max<uint32_t>(1, s->n_clusters) >= 192;
    const bool i8_shape = (s->sdim % 256) == 0 && !(flags & PQV_LAYOUT_ROW_ORDER) && s->n > 0;
    bool built = false;
    {
        static const bool eager_norms = [] { const char *e = std::getenv("PQV_EAGER_NORMS"); return e && *e == '1'; }();
        if (build_now && i8_shape && !eager_norms) {
            s->i8_ok = true;                                   // (tentatively: screen_op must see it)
            if (screen_op(s) == 2) {
                const int rc = ensure_blocked_copy(s, 2, s->stream);
                if (rc == PQV_OK) built = true;
                else if (rc != kNotFinite) { delete s; return rc; }
            }
            if (!built) s->i8_ok = false;
        }
    }
    mark("int8 copy first");
    if (!built) {
        if (int rc = ensure_row_norms(s, s->stream)) { delete s; return rc; }
        mark("row norms + maximum");
        s->i8_ok = s->f16_ok && i8_shape;
        if (build_now) {
            if (int rc = ensure_blocked_copy(s, screen_op(s), s->stream)) { delete s; return rc; }
        }
    }
    S_TRY(hipStreamSynchronize(s->stream));
    mark("blocked operand copy");
    if (!(flags & PQV_LAYOUT_ROW_ORDER) && corpus->owned &&
        ((flags & PQV_RELEASE_ROW_ORDER) || ((flags & PQV_RELEASE_IF_COPIED) && !s->images_only))) {
        (void)hipFree(corpus->d_rows);
        corpus->d_rows = nullptr;
    }
#undef S_TRY
    mark("release / epilogue");
    *out = s;
    return PQV_OK;
}
static int ensure_cosine(const pqv_searcher *s);
// PQV_PREPARE_COSINE: the cosine layout now; a searcher whose layout cannot be built is not returned
static int prepare_cosine(uint32_t flags, pqv_searcher **out) {
    if (!(flags & PQV_PREPARE_COSINE) || !*out) return PQV_OK;
    int rc;
    {
        std::lock_guard<std::mutex> lock((*out)->mu);
        rc = ensure_cosine(*out);
    }
    if (rc) { pqv_searcher_free(*out); *out = nullptr; }
    return rc;
}
extern "C" int pqv_searcher_create(const pqv_index *index, pqv_corpus *corpus, uint32_t flags,
                                   pqv_searcher **out) {
    return guard([&] {
        if (int rc = pqv_searcher_create_impl(index, corpus, flags, out)) return rc;
        return prepare_cosine(flags, out);
    });
}

// A table of indexed files (pqv.h: pqv_table_searcher_create): the files' indexes concatenated into ONE index -- centroid tables
// and inverted lists appended file after file, each file's rows shifted by its row_base -- and an ordinary searcher over it (the
// IVF-ordered layout, operand images and norms exactly as for one index); the per-file centroid segments make the probe count
// nprobe per file.
static int pqv_table_searcher_create_impl(const pqv_index *const *indexes, uint32_t n_files, const uint64_t *row_base,
                                          pqv_corpus *corpus, uint32_t flags, pqv_searcher **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!indexes || !row_base || !corpus) return fail(PQV_ERR_INVALID, "indexes/row_base/corpus must not be NULL");
    if (n_files == 0) return fail(PQV_ERR_INVALID, "a table needs at least one indexed file");
    uint64_t kc_total = 0, rows_end = 0;
    for (uint32_t f = 0; f < n_files; ++f) {
        const pqv_index *ix = indexes[f];
        const std::string fs = std::to_string(f);
        if (!ix) return fail(PQV_ERR_INVALID, "index of file " + fs + " must not be NULL");
        if (ix->dim != indexes[0]->dim)
            return fail(PQV_ERR_INVALID, "index dimension " + std::to_string(ix->dim) + " of file " + fs +
                                             " does not match dimension " + std::to_string(indexes[0]->dim) + " of file 0");
        if (ix->dim != corpus->dim)
            return fail(PQV_ERR_INVALID, "index dimension " + std::to_string(ix->dim) + " of file " + fs +
                                             " does not match corpus dimension " + std::to_string(corpus->dim));
        uint64_t n_f = 0;                              // the file's extent: its row bound (ids a remove left free stay the file's)
        if (!ix->row_bound(&n_f)) return PQV_ERR_HIP;
        if (f > 0 && row_base[f] < rows_end)
            return fail(PQV_ERR_INVALID, "row range of file " + fs + " starts at " + std::to_string(row_base[f]) +
                                             ", inside the rows of the files before it (ranges must be increasing and disjoint)");
        if (row_base[f] > corpus->n || n_f > corpus->n - row_base[f])
            return fail(PQV_ERR_INVALID, "row range [" + std::to_string(row_base[f]) + ", " + std::to_string(row_base[f] + n_f) +
                                             ") of file " + fs + " lies outside the corpus of " + std::to_string(corpus->n) + " rows");
        rows_end = row_base[f] + n_f;
        kc_total += ix->n_clusters;
    }
    if (rows_end >= 0xFFFFFFFFull) return fail(PQV_ERR_INVALID, "a table's rows must stay below 2^32 - 1 (0xFFFFFFFF marks an empty slot)");
    if (kc_total > 0xFFFFFFFFull) return fail(PQV_ERR_INVALID, "a table's clusters must stay below 2^32");
    pqv_index all;
    all.dim = indexes[0]->dim;
    all.n_clusters = static_cast<uint32_t>(kc_total);
    std::vector<uint32_t> seg_off(n_files + 1, 0);
    uint32_t seg_max = 0;
    all.list_off.reserve(kc_total + 1);
    all.list_off.push_back(0);
    for (uint32_t f = 0; f < n_files; ++f) {
        const pqv_index *ix = indexes[f];
        const std::vector<uint32_t> *rv = ix->rows->get();
        if (!rv) return PQV_ERR_HIP;
        uint64_t bound_f = 0;
        if (!ix->row_bound(&bound_f)) return PQV_ERR_HIP;
        const uint64_t o = all.list_off.back();
        all.centroids.insert(all.centroids.end(), ix->centroids.begin(), ix->centroids.end());
        for (uint32_t c = 0; c < ix->n_clusters; ++c) all.list_off.push_back(o + ix->list_off[c + 1]);
        const uint32_t rb = static_cast<uint32_t>(row_base[f]);
        for (uint32_t r : *rv) {
            if (r >= bound_f) return fail(PQV_ERR_INVALID, "index row id out of range for file " + std::to_string(f));
            all.list_rows.push_back(rb + r);
        }
        seg_off[f + 1] = seg_off[f] + ix->n_clusters;
        seg_max = std::max(seg_max, ix->n_clusters);
    }
    all.rows->n = all.list_rows.size();
    pqv_searcher *s = nullptr;
    if (int rc = pqv_searcher_create_impl(&all, corpus, flags, &s)) return rc;
    s->n_files = n_files;
    s->seg_off = std::move(seg_off);
    s->row_base.assign(row_base, row_base + n_files);
    s->seg_max_kc = seg_max;
    s->rr_cap = (flags & PQV_TABLE_CAP_ROUND_ROBIN) != 0;
    const std::vector<uint64_t> seg_off64(s->seg_off.begin(), s->seg_off.end());
    hipError_t e = s->d_seg_off.alloc(s->seg_off.size() * sizeof(uint32_t));
    if (e == hipSuccess) e = s->d_seg_off64.alloc(seg_off64.size() * sizeof(uint64_t));
    if (e == hipSuccess) e = hipMemcpy(s->d_seg_off.p, s->seg_off.data(), s->seg_off.size() * sizeof(uint32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(s->d_seg_off64.p, seg_off64.data(), seg_off64.size() * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        delete s;
        return fail(e == hipErrorOutOfMemory ? PQV_ERR_OOM : PQV_ERR_HIP, std::string("segment table upload: ") + hipGetErrorString(e));
    }
    *out = s;
    return PQV_OK;
}
extern "C" int pqv_table_searcher_create(const pqv_index *const *indexes, uint32_t n_files, const uint64_t *row_base,
                                         pqv_corpus *corpus, uint32_t flags, pqv_searcher **out) {
    return guard([&] {
        if (int rc = pqv_table_searcher_create_impl(indexes, n_files, row_base, corpus, flags, out)) return rc;
        return prepare_cosine(flags, out);
    });
}
extern "C" int pqv_searcher_files(const pqv_searcher *s, uint32_t *n_files, uint64_t *row_base, uint32_t *cluster_base) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    const uint32_t n = s->n_files ? s->n_files : 1;
    if (n_files) *n_files = n;
    for (uint32_t f = 0; f < n; ++f) {
        if (row_base) row_base[f] = s->n_files ? s->row_base[f] : 0;
        if (cluster_base) cluster_base[f] = s->n_files ? s->seg_off[f] : 0;
    }
    return PQV_OK;
}

// The cosine layout of a searcher (pqv.h: PQV_COSINE), under s->mu: the centroid table and the column normalised on the device
// (normalize_rows_kernel), then an ordinary searcher over them that shares the index' lists and takes the layout `s` has -- rows
// read through the list order from the normalised row-order copy (images-only IVF, ROW_ORDER), or an IVF-ordered copy of its own,
// after which its row-order copy is released: one more f32 copy of the column either way -- with the images, norms and per-list
// centres its creation builds from those rows.  A table's file segments are copied over.  Any failure leaves `s` as it was.
static int ensure_cosine(const pqv_searcher *s) {
    if (s->cos) return PQV_OK;
    if (int rc = use_device(s->device)) return rc;
    const uint32_t kc = s->n_clusters, dim = s->dim;
    pqv_index ni;
    ni.dim = dim; ni.n_clusters = kc; ni.list_off = s->h_list_off; ni.rows = s->h_rows;
    try { ni.centroids.resize(static_cast<size_t>(kc) * dim); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
    std::unique_ptr<pqv_corpus> nc(new (std::nothrow) pqv_corpus());
    if (!nc) return fail(PQV_ERR_OOM, "host allocation failed");
    const pqv_corpus *src = s->corpus;
    nc->device = s->device; nc->dim = dim; nc->n = nc->capacity = src->n; nc->owned = true;
    {
        DevBuf d_nc;
        HIP_TRY(d_nc.alloc(std::max<size_t>(1, ni.centroids.size()) * sizeof(float)));
        HIP_TRY(pqv::launch_normalize_rows(s->d_centroids.as<float>(), dim, nullptr, kc, dim, d_nc.as<float>(), s->stream));
        HIP_TRY(hipMalloc(reinterpret_cast<void **>(&nc->d_rows), std::max<size_t>(1, src->n) * dim * sizeof(float)));
        if (src->d_rows) {
            HIP_TRY(pqv::launch_normalize_rows(src->d_rows, dim, nullptr, src->n, dim, nc->d_rows, s->stream));
        } else {
            // the caller's row-order copy was released (PQV_RELEASE_ROW_ORDER): the searcher's own IVF-ordered copy is the source, its
            // storage rows go back to their file rows (zero padding adds nothing to the chain); rows of no list stay zero
            HIP_TRY(hipMemsetAsync(nc->d_rows, 0, std::max<size_t>(1, src->n) * dim * sizeof(float), s->stream));
            HIP_TRY(pqv::launch_normalize_rows(s->d_mat, s->sdim, s->d_final_ids, s->n, dim, nc->d_rows, s->stream));
        }
        if (!ni.centroids.empty())
            HIP_TRY(hipMemcpyAsync(ni.centroids.data(), d_nc.p, ni.centroids.size() * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    const uint32_t flags = s->images_only ? 0u : s->d_row_of ? PQV_LAYOUT_ROW_ORDER : PQV_RELEASE_ROW_ORDER;
    pqv_searcher *c = nullptr;
    if (int rc = pqv_searcher_create_impl(&ni, nc.get(), flags, &c)) return rc;
    std::unique_ptr<pqv_searcher> cu(c);
    c->opt = s->opt;
    c->timing = s->timing;
    if (s->n_files) {
        c->n_files = s->n_files; c->seg_off = s->seg_off; c->row_base = s->row_base; c->seg_max_kc = s->seg_max_kc; c->rr_cap = s->rr_cap;
        HIP_TRY(c->d_seg_off.alloc(s->d_seg_off.bytes));
        HIP_TRY(c->d_seg_off64.alloc(s->d_seg_off64.bytes));
        HIP_TRY(hipMemcpy(c->d_seg_off.p, s->d_seg_off.p, s->d_seg_off.bytes, hipMemcpyDeviceToDevice));
        HIP_TRY(hipMemcpy(c->d_seg_off64.p, s->d_seg_off64.p, s->d_seg_off64.bytes, hipMemcpyDeviceToDevice));
    }
    s->cos_corpus = std::move(nc);
    s->cos = std::move(cu);
    return PQV_OK;
}

// CandidateCursor::next_batch(max_candidates) of a fresh cursor over files with counts[f] candidates (access.rs:214-242), as
// per-file tallies in closed form: L = the largest level with S(L) = sum_f min(counts[f], L) <= max_candidates, every file keeps
// min(counts[f], L), and the first max_candidates - S(L) files with more than L candidates one more.  max_candidates == 0 or
// >= the total: no cap.  merge_probe_seg_kernel (table_quota) computes the same numbers on the device.
static void round_robin_quota(const uint64_t *counts, uint32_t n_files, uint64_t max_candidates, uint64_t *quota) {
    // S(L), saturating at 2^64 - 1 (it is only compared with max_candidates)
    auto level_sum = [&](uint64_t L) {
        uint64_t sum = 0;
        for (uint32_t f = 0; f < n_files; ++f) {
            const uint64_t v = std::min(counts[f], L);
            sum = sum + v < sum ? ~0ull : sum + v;
        }
        return sum;
    };
    const uint64_t max_c = n_files ? *std::max_element(counts, counts + n_files) : 0;
    if (max_candidates == 0 || level_sum(max_c) <= max_candidates) {
        std::copy(counts, counts + n_files, quota);
        return;
    }
    uint64_t lo = 0, hi = max_c, s_lo = 0;      // S(lo) <= M < S(hi)
    while (hi - lo > 1) {
        const uint64_t mid = lo + (hi - lo) / 2, sm = level_sum(mid);
        if (sm <= max_candidates) { lo = mid; s_lo = sm; } else hi = mid;
    }
    uint64_t rem = max_candidates - s_lo;
    for (uint32_t f = 0; f < n_files; ++f) {
        quota[f] = std::min(counts[f], lo);
        if (counts[f] > lo && rem) { quota[f] += 1; --rem; }
    }
}
extern "C" int pqv_round_robin_quota(const uint64_t *counts, uint32_t n_files, uint64_t max_candidates, uint64_t *quota) {
    if (n_files == 0) return PQV_OK;
    if (!counts || !quota) return fail(PQV_ERR_INVALID, "counts/quota must not be NULL");
    return guard([&] { round_robin_quota(counts, n_files, max_candidates, quota); return PQV_OK; });
}

extern "C" void pqv_searcher_free(pqv_searcher *s) {
    if (!s) return;
    (void)hipSetDevice(s->device);
    delete s;
}

namespace {

// probed lists per query: min(nprobe, n_clusters), on a table searcher the sum of min(nprobe, kc_f) over its files
uint32_t probe_count(const pqv_searcher *s, uint32_t nprobe) {
    if (!s->n_files) return std::min<uint32_t>(nprobe, s->n_clusters);
    uint64_t P = 0;
    for (uint32_t f = 0; f < s->n_files; ++f) P += std::min<uint32_t>(nprobe, s->seg_off[f + 1] - s->seg_off[f]);
    return static_cast<uint32_t>(std::min<uint64_t>(P, 0xFFFFFFFFull));
}

// a round-robin capped table on the host: the end of candidates of each of a query's P probed lists (clusters, file after file:
// min(nprobe, kc_f) of file f), as merge_probe_seg_kernel writes them to SegProbeArgs::pair_end
void table_pair_ends(const pqv_searcher *s, const std::vector<uint32_t> &clusters, uint32_t nprobe, uint64_t max_candidates,
                     std::vector<uint64_t> &end) {
    const uint32_t F = s->n_files;
    std::vector<uint64_t> cnt(F, 0), quota(F);
    size_t j = 0;
    for (uint32_t f = 0; f < F; ++f) {
        const uint32_t kf = std::min<uint32_t>(nprobe, s->seg_off[f + 1] - s->seg_off[f]);
        for (uint32_t i = 0; i < kf && j < clusters.size(); ++i, ++j) cnt[f] += s->h_list_off[clusters[j] + 1] - s->h_list_off[clusters[j]];
    }
    round_robin_quota(cnt.data(), F, max_candidates, quota.data());
    end.assign(clusters.size(), 0);
    uint64_t fb = 0;
    j = 0;
    for (uint32_t f = 0; f < F; ++f) {
        const uint32_t kf = std::min<uint32_t>(nprobe, s->seg_off[f + 1] - s->seg_off[f]);
        for (uint32_t i = 0; i < kf && j < clusters.size(); ++i, ++j) end[j] = fb + quota[f];
        fb += cnt[f];
    }
}

// stream_kernel's split of a pass over (query, list) pairs: enough blocks to fill the chip (~8192), lists cut into 256-row multiples
void stream_split(uint64_t max_len, uint64_t pairs, uint32_t &rows_per_block, uint32_t &blocks_per_list) {
    const uint64_t bpl = std::max<uint64_t>(1, std::min<uint64_t>((8192 + pairs - 1) / pairs, (max_len + 255) / 256));
    const uint64_t rpb = ((max_len + bpl - 1) / bpl + 255) / 256 * 256;
    rows_per_block = static_cast<uint32_t>(rpb);
    blocks_per_list = static_cast<uint32_t>((max_len + rpb - 1) / rpb);
}

struct TopkPlan {
    uint32_t np;            // effective nprobe
    uint32_t probe_bpl;     // blocks over the centroid matrix
    uint32_t probe_kpart;   // entries per partial list of the probe pass (np, or 64 unsorted from probe_rows_kernel)
    bool probe_rows;        // batched probe_rows_kernel instead of the per-query stream_kernel
    bool probe_screen;      // ... screened: probe_screen_kernel + probe_resolve_kernel write the same partial lists
    uint32_t rr_rows_per_block, rr_bpl;
    uint32_t n_part_probe, n_part_rr;
    bool tile;              // batched cluster-major tiles instead of one stream per (query, list)
    uint32_t max_groups;
    bool filter;            // tile path with the MFMA lower-bound screen
    uint32_t seed_rows, filter_bpl;
    bool f16;               // wide path with f16 operands (dim % 128 == 0, queries staged in LDS)
    bool i8;                // wide path with int8 operands (dim % 256 == 0, 8-wave blocks)
    bool quad;              // filter: wide_filter_kernel (quad_width queries per block); else tile_filter_kernel
    uint32_t filter_rows_per_block, max_quads, quad_width;
    uint32_t block_waves;   // wide kernel: waves per block (4, or 8 sharing one staged quad on a whole CU)
    uint32_t slots_per_pair;   // partial lists per (query, probe rank)
    uint32_t wide_width;    // > 0: quads of 97..wide_width pairs go to the wide-quad instance (its own item table)
    uint32_t wide_rows_per_block, wide_bpl;
    bool list_once;         // the wide table's quads hold up to wide_width (<= 1024) pairs of ONE list and run in list_filter_kernel
};

// Exact refinement of the seed threshold (SeedRefine): where survivors are expensive (rows of >= 256 dims; C2, 128 dims:
// 7.18 -> 7.04 M QPS with it).  Any batch size: one uniform C3 query pays 7 us for it (256 -> 263), but one query on the
// Gaussian-mixture set overflows its candidate buffer without it (282 -> 500 us).
// candidate-buffer entries per query: survivors of the screen grow with k (C3: 240 at k 10 with the refined first
// threshold, 810 at k 32, 2100 at k 100 -- and a query that overflows its buffer falls back to the per-wave sorted lists)
static uint32_t cand_cap_for(const pqv_searcher *s, uint32_t k) {
    return std::max<uint32_t>(s->opt.cand_cap ? s->opt.cand_cap : (k > 32 ? 8192u : 2048u), k);
}
// Deferred exact evaluation (TileArgs::cand_lb): pays where the exact evaluations are most of the screen kernel's time -- long
// lists of survivors, i.e. large k (the reference's bench shape, 1 M x 1024 at K = 100: 1226 evaluations per query in the
// filter -> 633 after it, screen kernel 2.14 -> 0.95 ms).  At k = 10 the streaming waves hide their evaluations behind each
// other and the extra launches cost more than they save (C3: 1.08 + 0.73 ms of screen either way), so the deferred form is
// compiled into the k > 64 instances of the kernel only (S > 1) and those always use it (PQV_DEFER=0: never).
// k <= 64: only where a wave's own evaluations are a large part of its short life -- lists of a few tiles per wave of long
// rows (int8 images of >= 512 dims; the two-instance form of batches).  With 1024 lists of 768-dim rows and k = 10, q/s
// deferred against in-filter: 488 rows per list 1.79 against 1.49 M, 976: 1.63 / 1.50 M, 2441: 1.29 / 1.20 M, 4883:
// 0.83 / 0.91 M, 9766 (C3): equal at best -- hence mean list <= 3072 rows.  128-dim rows cost less to evaluate than to
// defer (C2 7.8 -> 6.8 M, its 1000-list variant 5.9 -> 5.5 M).
static bool defer_on(const pqv_searcher *s, uint32_t nq, uint32_t k, const TopkPlan &p) {
    if (s->opt.defer == 0) return false;
    if (k > 64) return true;                    // (the kernels carry the deferred form in their k > 64 instances ...)
    const uint64_t mean_len = s->n / std::max<uint32_t>(1, s->n_clusters);
    // (... and in the DEFP instances of the int8 two-blocks-per-CU form: launch_filter_s)
    // (round 5, 768-dim rows, q/s deferred against in-filter on the final kernels -- uniform: 488-row lists 2.14 / 1.68 M, 976: 2.03 /
    //  1.72 M, 2441: 1.45 / 1.27 M; Gaussian mixture: 488: 2.25 / 2.30 M, 976: 1.87 / 1.78 M, 2441: 1.14 / 1.22 M -- on clustered
    //  query loads the upper-bound counting loosens the running thresholds and the gain is gone from ~1500-row lists on: there the
    //  previous batch's shape (prefer_regular: most popular lists probed by hundreds of queries) switches the form off)
    if (s->opt.defer != 2 && mean_len > 1536 && prefer_regular(s)) return false;
    return nq >= 8 && p.i8 && p.block_waves == 4 && p.quad_width == 96 && s->sdim >= 512 && (s->opt.defer == 2 || mean_len <= 3072);
}
// ... on the wide screened path, where a query's candidate buffer has room for the bounds
static bool defer_route(const pqv_searcher *s, uint32_t nq, uint32_t k, const TopkPlan &p) {
    return defer_on(s, nq, k, p) && cand_cap_for(s, k) <= 8192;
}
static bool seed_refine_on(const pqv_searcher *s, uint32_t nq, uint32_t k) {
    (void)nq;
    return s->opt.seed_refine && (!s->d_row_of || s->images_only) && (s->sdim % 32) == 0 && k <= 16 && (s->opt.seed_refine > 1 || s->sdim >= 256);
}
// exact_stream: a masked call -- the per-(query, list) stream whatever the options say (the screened paths' thresholds come from
// sampled rows the mask may exclude)
TopkPlan plan_topk(const pqv_searcher *s, uint32_t nq, uint32_t nprobe, uint32_t k = 1, int metric = 0, bool exact_stream = false) {
    TopkPlan p{};
    const pqv_searcher::Opts &o = s->opt;
    if (metric == PQV_DOT) exact_stream = true;     // (pqv.h: always the exact stream, whatever the options say)
    p.np = probe_count(s, nprobe);
    // probe pass: every block scans 256 centroids (64 per wave)
    p.probe_bpl = (s->n_clusters + 255) / 256;
    p.n_part_probe = p.probe_bpl * pqv::waves_per_block();
    // (a handful of queries: the per-query stream over the table is the shorter chain -- 26 against 31 us for one query)
    // (it writes every centroid key of every query: beyond 2 GiB of that scratch -- hundreds of thousands of centroids
    //  times tens of thousands of queries in one device call -- the per-query stream probe takes over)
    p.probe_rows = s->opt.probe_rows && s->kc_pad != 0 && (nq >= 8 || s->opt.probe_rows > 1) &&
                   static_cast<uint64_t>(nq) * s->kc_pad * 12 <= (2ull << 30);
    if (metric == PQV_DOT) p.probe_rows = false;    // (probe_rows_kernel is L2 arithmetic: dot_stream_kernel over the centroid matrix)
    // the screened form: where the contraction pays.  Measured on MI355X, 768 dims, nprobe 32, kernel time per batch in us
    // (rocprofv3 kernel trace, 4 calls each): probe_rows_kernel at 32 / 64 / 128 / 256 queries -- 1024 centroids 31.8 / 32.8 / 38.5 /
    // 40.4, 256 centroids 36.3 / 35.5 / 36.6 / 36.2 (a chain of 192 row loads whatever the batch); the screened route at all eight
    // shapes -- query images 4-6 + probe_screen_kernel 6.9-7.6 + probe_resolve_kernel 16.0-16.6 = 27-31.  From 128 queries on the
    // gain (8-12 us) is worth two more launches; below, it is 2-8 us of kernel time against them and the exact kernel stays.
    // Fewer than 256 centroids were not measured: they leave the 64 x 64 tiles a handful of blocks, and keep the exact kernel.
    // With np beyond kc / 4 (every-list parity runs, expanding searches that probe far) most centroids are contenders.
    p.probe_screen = p.probe_rows && s->ps.ok && o.probe_screen && !s->n_files && p.np >= 1 && p.np <= s->n_clusters / 4 &&
                     (o.probe_screen > 1 || (nq >= 128 && s->n_clusters >= 256));
    p.probe_kpart = p.probe_rows ? 64u : p.np;
    if (s->n_files && !p.probe_rows) {
        // table, stream_kernel probe: one list per file (no block straddles two files), the nprobe nearest of a file kept per partial list
        p.probe_bpl = (s->seg_max_kc + 255) / 256;
        p.n_part_probe = s->n_files * p.probe_bpl * pqv::waves_per_block();
        p.probe_kpart = std::min<uint32_t>(nprobe, s->seg_max_kc);
    }
    // re-rank: enough blocks to fill 256 CUs several times over, few enough partial lists
    const uint64_t max_len = std::max<uint64_t>(1, s->max_list_len);
    const uint64_t pairs = std::max<uint64_t>(1, static_cast<uint64_t>(nq) * p.np);
    // Tile path: worth it once several queries share a cluster (each streamed row is then
    // reused by up to TILE_QB queries).  k <= 256; REF4 order only.
    p.tile = metric == PQV_L2SQ_REF4 && k <= 256 && pairs >= 4ull * s->n_clusters;
    // ... except where the wide screened kernels apply (5.1c): they read the f16 copy of a list instead of its f32
    // rows and skip the exact arithmetic, which beats the streaming kernel at EVERY batch size -- one query on C2
    // 123 -> 78 us, on C3 2.0 -> 0.34 ms; 32 queries on C3 15.8 -> 2.2 ms
    const uint64_t mean_len = s->n / std::max<uint32_t>(1, s->n_clusters);
    const bool wide_ok = o.filter_variant == 0 && wide_path_possible(s);
    // (round 3: lists down to 192 rows -- the reference's default n_clusters = ceil(sqrt(n)) gives lists of sqrt(n) rows,
    //  index.rs:161-167 -- with a threshold sample that shrinks with them)
    const bool wide_any_batch = metric == PQV_L2SQ_REF4 && o.tile_filter && k <= 128 && wide_ok && mean_len >= 192;
    if (wide_any_batch) p.tile = true;
    if (o.rerank_mode == 1) p.tile = false;
    if (o.rerank_mode == 2) p.tile = metric == PQV_L2SQ_REF4 && k <= 256;
    if (exact_stream) p.tile = false;
    if (p.tile) {
        const uint64_t est_groups = std::max<uint64_t>(1, pairs / pqv::TILE_QB);
        // Rows per block: long enough to amortise a block's setup and top-k warm-up, short
        // enough that imbalanced lists do not leave a tail (measured optimum ~1.5 k on C2/C3);
        // shrink only when that would leave the GPU with too few blocks.
        const uint64_t tile_rows = o.tile_rows ? o.tile_rows : 1536;
        uint64_t rpb = std::min<uint64_t>(tile_rows, (max_len + 255) / 256 * 256);
        while (rpb > 256 && est_groups * ((max_len + rpb - 1) / rpb) < 2048) rpb -= 256;
        p.rr_rows_per_block = static_cast<uint32_t>(rpb);
        // threshold sample: 256 rows per probed list, 512 for lists of >= 4096 rows (survivors per query halve,
        // the sampling pass doubles: C2 0.246 -> 0.226 ms, C3 7.99 -> 7.58 ms)
        // short lists: a third of the mean list, in 64-row tiles
        p.seed_rows = o.seed_rows ? std::max<uint32_t>(64, o.seed_rows / 64 * 64)
                                  : (mean_len >= 4096 ? 512 : mean_len >= 768 ? 256 : static_cast<uint32_t>(std::max<uint64_t>(64, mean_len / 3 / 64 * 64)));
        // k <= 128 (the running-threshold counters are 8 bits wide, the candidate buffers 2048 entries); the wide
        // kernel pays from lists of three seed windows on -- measured on the reference's own bench shape, 1000-row
        // lists at K = 100: 99 k -> 243 k QPS; the one-group kernel (row-order layout, dim % 64 != 0) keeps k <= 32
        // and wins from 4 pairs per cluster on 10 k-row lists: 0.45 -> 0.25 ms at 64 queries, 0.52 -> 0.34 at 256
        p.filter = o.tile_filter && k <= (wide_ok ? 128u : 32u) && pairs >= (wide_ok ? 0ull : 4ull) * s->n_clusters &&
                   mean_len >= (wide_ok ? 3ull : 16ull) * p.seed_rows;
        if (o.tile_filter == 2) p.filter = max_len > 4ull * p.seed_rows && k <= 256;   // forced
        if (p.filter) {
            p.quad = wide_ok;
            const int op = p.quad ? screen_op(s, k) : 0;
            p.i8 = op == 2;
            p.f16 = op == 1;
            // Quad width = queries that share one pass over a list.  f32 operands: 64 (dim <= 128) or 32 staged in
            // LDS, longer rows read a blocked per-quad copy from global memory.  f16 operands: everything the LDS of
            // a CU holds next to the queues -- 144 KB: 128 queries up to 512 dims, 96 at 768, 64 at 1024 -- in ONE
            // 8-wave block per CU, because how often a list is streamed is what bounds long rows (C3, PMC: the
            // 32-query form moves 41 GB per step through the fabric at 6.8 TB/s for 15 GB of distinct rows).
            p.block_waves = 4;
            if (p.i8) {             // int8 images: a byte per value -- 128 queries up to 1024 dims, 96 at 1536, 64 at 2048
                // Up to 1024 dims a 64-query quad is <= 64 KB (96 queries <= 72 KB up to 768 dims), so TWO 4-wave blocks
                // share a CU: the blocks are at different phases (staging / MFMA screen / exact evaluations) and fill
                // each other's stalls, which one 8-wave block in lockstep cannot.  C3, kernel time in one run: one
                // 8-wave block of 96 queries 2.45 ms (12.2 GB through the fabric), two 4-wave blocks of 64 queries 2.36 ms
                // (15.3 GB at 6.5 TB/s: bandwidth-bound), two of 96 queries 2.21 ms.  Longer rows: one 8-wave block.
                p.block_waves = (o.wide_waves != 8 && 64ull * s->sdim <= 65536) ? 4 : 8;
                // (the 128-query form keeps 128 accumulator registers per lane and spills inside the K loop: 96 by default)
                const uint32_t fit = static_cast<uint32_t>(std::min<uint64_t>(128, 147456ull / s->sdim / 32 * 32));
                p.quad_width = std::min<uint32_t>(96, fit);
                if (o.quad_width && (o.quad_width % 32) == 0 && o.quad_width >= 64 && o.quad_width <= fit) p.quad_width = o.quad_width;
                // (a batch that leaves most quads with a few queries -- a single query above all -- takes the 64-query
                //  form: no spills, 250 against 290 us for one C3 query)
                if (p.block_waves == 4)
                    p.quad_width = (o.quad_width != 64 && 96ull * s->sdim <= 73728 && (o.quad_width == 96 || pairs >= 16ull * s->n_clusters)) ? 96 : 64;
            } else if (p.f16) {
                const uint64_t per_q = static_cast<uint64_t>(s->sdim) * (s->sdim <= 128 ? 6 : 2);     // f16 image (+ f32 original)
                const uint32_t fit8 = static_cast<uint32_t>(std::min<uint64_t>(128, 147456 / per_q / 32 * 32));
                // two 4-wave blocks of 96 queries per CU where 96 queries fit 72 KB (up to 128 dims with the f32 originals,
                // up to 384 without): C2 7.15 -> 8.02 M QPS against one 8-wave block of 128 (0.151 -> 0.133 ms kernel
                // time; 5.1f's overlap of two blocks' phases).  Longer rows: one 8-wave block.
                const bool two96 = 96ull * per_q <= 73728;
                const uint32_t fit4 = two96 ? 96 : s->sdim <= 256 ? 64 : 32;
                int waves = o.wide_waves == 4 || o.wide_waves == 8 ? o.wide_waves : two96 ? 4 : 8;
                if (fit8 < 64) waves = 4;
                // (a call of a few queries has no quad of more: the 4-wave form -- 32-query quads of long rows, 64 KB, two blocks per
                //  CU -- loses nothing to a second pass and its blocks are not mostly fixed cost; one query at K = 100 on 1 M x 1024:
                //  330 -> 277 us per call against the 8-wave block of 64; from 8 queries on the 8-wave form is as good or better)
                if (o.wide_waves != 8 && nq <= 4 && !two96 && fit4 >= 32) waves = 4;
                p.block_waves = static_cast<uint32_t>(waves);
                p.quad_width = waves == 8 ? fit8 : fit4;
                // (a requested width the chosen form has no instantiation for is ignored, never an error at launch: the
                //  whole-tile-prefetch form of rows <= 128 dims exists for 64 and 96 queries only)
                const bool pf_form = waves == 4 && s->sdim <= 128;
                if (o.quad_width && (o.quad_width % 32) == 0 && o.quad_width <= p.quad_width && (waves == 4 || o.quad_width >= 64) &&
                    !(pf_form && o.quad_width == 32))
                    p.quad_width = o.quad_width;
            } else {
                p.quad_width = s->sdim <= 128 ? 64 : 32;
            }
            uint64_t r = rpb;
            if (p.quad) {
                // a wave's fixed cost (staging the quad's queries, the last partial batch of exact evaluations) is
                // about half its time at 1536 rows per 4-wave block, and the lists are cut into equal pieces, so
                // longer blocks pay: measured optimum 2304 on C2 (0.221 -> 0.193 ms) and C3 (6.63 -> 6.35 ms);
                // the 8-wave blocks (one per CU) measured best at 3072 on C3 (2.60 -> 2.51 ms against 4608)
                // the two-block int8 form is flat between 1280 and 5120 on the item grid (C3: 2.19 / 2.20 / 2.16 ms at 1280 /
                // 1792 / 3072; C4 shard: 2.77 / 2.69 / 2.71)
                const uint64_t wide_rows = o.wide_rows >= 256 ? std::min<uint64_t>(o.wide_rows, 1u << 22) / 256 * 256
                                           : (p.block_waves == 8 || p.i8 || p.quad_width == 96) ? 3072ull : 2304ull;
                const uint64_t est_quads = std::max<uint64_t>(1, pairs / p.quad_width);
                const uint64_t min_blocks = o.min_blocks ? o.min_blocks : (p.block_waves == 8 ? 1024 : 2048);
                r = std::min<uint64_t>(wide_rows, (max_len + 255) / 256 * 256);
                while (r > 256 * (p.block_waves / 4) && est_quads * (p.quad_width / 16) * ((max_len + r - 1) / r) < min_blocks) r -= 256;
            }
            p.filter_rows_per_block = static_cast<uint32_t>(r);
            if (p.quad) {           // the screened pass covers the whole list; the seed rows are only sampled
                p.filter_bpl = static_cast<uint32_t>((max_len + r - 1) / r);
                p.rr_bpl = p.filter_bpl;
                p.slots_per_pair = p.block_waves * p.filter_bpl;
                // Lists that more than 96 queries of the batch probe (the long, popular ones: 36 % of C3's distinct probed
                // rows) would be streamed twice; a quad of up to 160 queries on 32-row tiles (same accumulator registers) in
                // one 8-wave block per CU reads them once.  Batches only (pairs >= 16 per list on average), work-item grid.
                // Round 6: list_filter_kernel instead -- the list's rows stationary in registers and ALL its pairs (one quad of up to 1024)
                // streamed past them, so a list is read ONCE however many queries probe it (clustered query loads: hundreds).  Not with
                // the deferred form (its survivors carry the wide_filter_kernel queue's raw scores).
                if (p.i8 && p.block_waves == 4 && p.quad_width == 96 && o.wide_quads && o.item_grid >= 1 && pairs >= 16ull * s->n_clusters) {
                    const bool deferred = defer_route(s, nq, k, p);
                    if (o.list_once && o.wide_quads != 2 && !deferred && (s->sdim % 256) == 0 && s->sdim <= 768 && k <= 256) {
                        p.list_once = true;
                        p.wide_width = std::min<uint32_t>(1024u, std::max<uint32_t>(192u, (nq + 63u) / 64u * 64u));
                        const uint64_t wr = o.wide_quad_rows >= 256 ? std::min<uint64_t>(o.wide_quad_rows, 1u << 22) / 256 * 256 : 2048ull;
                        p.wide_rows_per_block = static_cast<uint32_t>(std::min<uint64_t>(wr, (max_len + 255) / 256 * 256));
                        p.wide_bpl = static_cast<uint32_t>((max_len + p.wide_rows_per_block - 1) / p.wide_rows_per_block);
                        p.slots_per_pair = std::max(p.slots_per_pair, 4 * p.wide_bpl);
                    } else if (!(o.wide_quads == 1 && prefer_regular(s)) && 160ull * s->sdim <= 122880) {
                        p.wide_width = 160;
                        const uint64_t wr = o.wide_quad_rows >= 512 ? std::min<uint64_t>(o.wide_quad_rows, 1u << 22) / 256 * 256 : 8192ull;
                        p.wide_rows_per_block = static_cast<uint32_t>(std::min<uint64_t>(wr, (max_len + 255) / 256 * 256));
                        p.wide_bpl = static_cast<uint32_t>((max_len + p.wide_rows_per_block - 1) / p.wide_rows_per_block);
                        p.slots_per_pair = std::max(p.slots_per_pair, 8 * p.wide_bpl);
                    }
                }
            } else {                // narrow kernel: exact seed window (slot chunk 0), screened remainder
                p.filter_bpl = static_cast<uint32_t>((max_len - p.seed_rows + r - 1) / r);
                p.rr_bpl = 1 + p.filter_bpl;
                p.slots_per_pair = 4 * (1 + p.filter_bpl);
            }
        } else {
            p.filter_bpl = 0;
            p.rr_bpl = static_cast<uint32_t>((max_len + rpb - 1) / rpb);
            p.slots_per_pair = 4 * p.rr_bpl;
        }
        p.n_part_rr = p.np * p.slots_per_pair;
        p.max_quads = static_cast<uint32_t>(pairs / std::max<uint32_t>(16, p.quad_width) + std::min<uint64_t>(s->n_clusters, pairs));
        p.max_quads = (p.max_quads + 7) / 8 * 8;       // quad_xcd_remap
        p.max_groups = static_cast<uint32_t>(pairs / pqv::TILE_QB + std::min<uint64_t>(s->n_clusters, pairs));
        return p;
    }
    stream_split(max_len, pairs, p.rr_rows_per_block, p.rr_bpl);
    p.n_part_rr = p.np * p.rr_bpl * pqv::waves_per_block();
    return p;
}

// tables: the per-file cap of the reference (access.rs:214-242) is not one prefix of the file-major candidate sequence -- a
// table applies it only when created with PQV_TABLE_CAP_ROUND_ROBIN
int table_max_candidates(const pqv_searcher *s, uint64_t max_candidates) {
    if (s->n_files && max_candidates && !s->rr_cap)
        return fail(PQV_ERR_UNSUPPORTED, "max_candidates > 0 is not supported on a table searcher: cap per file with "
                                         "pqv_candidate_cursor over per-file searchers and merge their results");
    return PQV_OK;
}
// the kernels take per-pair candidate ends (SegProbeArgs::pair_end) instead of one cap
bool table_rr(const pqv_searcher *s, uint64_t max_candidates) { return s->n_files && s->rr_cap && max_candidates; }

// The probe's outputs, P lists per query: sc.s_probe / s_cand_base [nq * P] (probed lists nearest first, a table's file after file;
// their first candidate positions), sized nq * max(P, n_files): a table's stream probe first reads its per-file arguments there.
int ensure_probe_slots(const pqv_searcher *s, Scratch &sc, uint32_t nq, uint32_t np) {
    const size_t slots = static_cast<size_t>(nq) * std::max<uint32_t>(np, s->n_files);
    HIP_TRY(sc.s_probe.ensure(slots * sizeof(uint32_t)));
    HIP_TRY(sc.s_cand_base.ensure(slots * sizeof(uint64_t)));
    return PQV_OK;
}

// The device probe's scratch and the probe merge's common arguments (k = P, totals to s_ncand, positions below max_candidates).
// Made first: the caller's own fields may point into that scratch (and the fused one-query probe takes the same arguments).
// pm.stats stays unset: a call that counts its candidates sets it.
int probe_merge_args(const pqv_searcher *s, Scratch &sc, const TopkPlan &p, uint32_t nq, uint64_t max_candidates, pqv::MergeArgs &pm) {
    const size_t n_keys = static_cast<size_t>(nq) * p.n_part_probe * p.probe_kpart;
    HIP_TRY(sc.s_probe_keys.ensure(n_keys * sizeof(uint64_t)));
    HIP_TRY(sc.s_probe_vals.ensure(n_keys * sizeof(uint32_t)));
    if (int rc = ensure_probe_slots(s, sc, nq, p.np)) return rc;
    HIP_TRY(sc.s_ncand.ensure(static_cast<size_t>(nq) * sizeof(uint64_t)));
    pm.part_keys = sc.s_probe_keys.as<uint64_t>(); pm.part_vals = sc.s_probe_vals.as<uint32_t>();
    pm.nq = nq; pm.n_part = p.n_part_probe; pm.k_part = p.probe_kpart; pm.k = p.np;
    pm.list_off = s->d_list_off.as<uint64_t>();
    pm.probe = sc.s_probe.as<uint32_t>(); pm.cand_base = sc.s_cand_base.as<uint64_t>();
    pm.n_cand = sc.s_ncand.as<uint64_t>();
    pm.max_pos = max_candidates ? max_candidates : ~0ull;
    return PQV_OK;
}

// The centroid probe on the device (P <= 1024: the kernels' sorted lists): the distance pass, then the probe merge (a table: per
// file segment, merge_probe_seg_kernel).  pm: from probe_merge_args plus the caller's fields; zero_u32 / zero_n: scratch the
// distance pass zeroes on the way (the tile path's histogram).  With the round-robin cap (table_rr) the merge also writes
// sc.s_pair_end [nq * P]: every list's end of candidates, its file's quota.
int enqueue_probe(const pqv_searcher *s, Scratch &sc, const TopkPlan &p, const float *d_queries, uint32_t nq, uint32_t nprobe,
                  uint64_t max_candidates, const pqv::MergeArgs &pm, uint32_t *zero_u32, uint32_t zero_n, hipStream_t stream,
                  int metric = PQV_L2SQ_REF4) {
    using namespace pqv;
    uint64_t *keys = const_cast<uint64_t *>(pm.part_keys);
    uint32_t *vals = const_cast<uint32_t *>(pm.part_vals);
    if (p.probe_screen) {   // a batch, screened: f16 images of the queries, the contraction, exact chains for the contenders
        const pqv_searcher::ProbeScreen &ps = s->ps;
        HIP_TRY(sc.s_ps_q16.ensure(static_cast<size_t>(nq) * ps.dim_p * sizeof(uint16_t)));
        HIP_TRY(sc.s_ps_qn2.ensure(static_cast<size_t>(nq) * sizeof(float)));
        HIP_TRY(sc.s_ps_score.ensure(static_cast<size_t>(nq) * s->kc_pad * sizeof(float)));
        HIP_TRY(launch_center_normalize_f16(d_queries, s->d_ps_mu.as<float>(), nq, nq, s->dim, ps.dim_p, sc.s_ps_qn2.as<float>(), sc.s_ps_q16.p, stream));
        ProbeScreenArgs pr{};
        pr.q16 = sc.s_ps_q16.as<uint16_t>(); pr.c16 = s->d_ps_c16.as<uint16_t>(); pr.qn2 = sc.s_ps_qn2.as<float>(); pr.cn2 = s->d_ps_cn2.as<float>();
        pr.score = sc.s_ps_score.as<float>(); pr.queries = d_queries; pr.centroids = s->d_centroids.as<float>();
        pr.nq = nq; pr.kc = s->n_clusters; pr.kc_pad = s->kc_pad; pr.dim = s->dim; pr.dim_p = ps.dim_p; pr.np = p.np;
        pr.inv_cs = ps.inv_cs; pr.fn = ps.fn; pr.e1 = ps.e1; pr.e2s = ps.e2s; pr.kS = ps.kS; pr.lo_f = ps.lo_f; pr.hi_f = ps.hi_f;
        pr.part_keys = keys; pr.part_vals = vals;
        pr.zero_u32 = zero_u32; pr.zero_n = zero_n;
        pr.stats = s->d_ps_stats.as<unsigned long long>();
        HIP_TRY(launch_probe_screen(pr, stream));
        s->counters.kernel_launches += 2;       // (the callers count ONE distance pass and the merge: this route enqueues three launches in its place)
    } else if (p.probe_rows) {     // a batch: a lane per centroid, the chains of up to 8 queries in registers
        ProbeRowsArgs pr{};
        pr.cent_t = s->d_cent_t.as<float4>(); pr.queries = d_queries;
        pr.nq = nq; pr.kc = s->n_clusters; pr.kc_pad = s->kc_pad; pr.dim = s->dim;
        pr.part_keys = keys; pr.part_vals = vals;
        pr.zero_u32 = zero_u32; pr.zero_n = zero_n;
        HIP_TRY(launch_probe_rows(pr, stream));
    } else {                // the re-rank kernel over the centroid matrix, k = P (a table: min(nprobe, kc_f) per file)
        StreamArgs pa{};
        pa.mat = s->d_centroids.as<float>();
        if (s->n_files) {
            HIP_TRY(launch_seg_probe_fill(s->d_seg_off.as<uint32_t>(), s->n_files, nq, sc.s_probe.as<uint32_t>(), sc.s_cand_base.as<uint64_t>(), stream));
            pa.list_off = s->d_seg_off64.as<uint64_t>(); pa.probe = sc.s_probe.as<uint32_t>(); pa.cand_base = sc.s_cand_base.as<uint64_t>();
            pa.nprobe = s->n_files;
        } else {
            pa.single_begin = 0; pa.single_end = s->n_clusters;
            pa.nprobe = 1;
        }
        pa.queries = d_queries; pa.nq = nq; pa.dim = s->dim; pa.k = p.probe_kpart;
        pa.rows_per_block = 256; pa.blocks_per_list = p.probe_bpl;
        pa.max_pos = ~0ull; pa.metric = PQV_L2SQ_REF4;   // find_closest_centroids always uses index.rs:461
        pa.part_keys = keys; pa.part_vals = vals;
        pa.zero_u32 = zero_u32; pa.zero_n = zero_n;
        if (metric == PQV_DOT) {     // centroids ranked by (dist, id): the merges below use the keys for their order only
            pa.metric = PQV_DOT;
            HIP_TRY(launch_dot_stream(pa, nullptr, STREAM_TOPK, stream));
        } else
        HIP_TRY(launch_stream(pa, STREAM_TOPK, stream));
        if (s->n_files) s->counters.kernel_launches += 2;
    }
    if (!s->n_files) {
        HIP_TRY(launch_merge_probe(pm, stream));
        return PQV_OK;
    }
    SegProbeArgs g{};
    g.seg_off = s->d_seg_off.as<uint32_t>(); g.n_files = s->n_files; g.nprobe = nprobe;
    g.kmax = std::min<uint32_t>(nprobe, s->seg_max_kc);
    g.stream_parts = p.probe_rows ? 0u : p.probe_bpl * waves_per_block();
    if (table_rr(s, max_candidates)) {
        HIP_TRY(sc.s_pair_end.ensure(std::max<size_t>(1, static_cast<size_t>(nq) * p.np) * sizeof(uint64_t)));
        HIP_TRY(sc.s_file_cnt.ensure(static_cast<size_t>(nq) * s->n_files * sizeof(uint32_t)));
        g.max_cand = max_candidates; g.pair_end = sc.s_pair_end.as<uint64_t>(); g.file_cnt = sc.s_file_cnt.as<uint32_t>();
    }
    HIP_TRY(launch_merge_probe_seg(pm, g, stream));
    return PQV_OK;
}

// pqv_timing_read's four events of one call (probe start, re-rank start, re-rank stop, end), kept in s->ev; all null when
// timing is off
int timing_events(const pqv_searcher *s, hipEvent_t (&e)[4]) {
    for (hipEvent_t &x : e) x = nullptr;
    if (!s->timing) return PQV_OK;
    for (hipEvent_t &x : e) HIP_TRY(hipEventCreate(&x));
    s->ev.insert(s->ev.end(), e, e + 4);
    return PQV_OK;
}

// The routing decisions of one top-k batch, derived once from (searcher, plan, nq, k): what the stages of enqueue_topk branch on
// and what pqv_searcher_describe prints.  Everything below `screened` is false / 0 off the wide screened path.
struct TopkRoute {
    bool screened;          // the wide screen (p.tile && p.filter && p.quad): wide_seed_kernel, seed select, wide_filter_kernel
    int operand;            // its operands, as the index of the blocked copy it reads: 0 f32, 1 f16, 2 int8
    bool fused_probe;       // one query, no table: probe, probe merge, bucketing and quantisation in ONE block (probe_single_kernel)
    bool single_bucket;     // one query: the probe merge writes the bucketing itself (MergeArgs::sq_*), no pair sort
    bool items;             // work-item tables (quad x row chunk that exists) instead of the 2-D grid (which tables of > 2^24 entries keep)
    bool wide;              // the wide-quad instance beside the regular quads, with an item table of its own
    uint32_t max_items, wide_max_items;
    bool q_global;          // rows too long to stage a quad's queries in LDS: blocked copy per quad in global memory
    bool seed_tail;         // one query: the seed kernel's last block selects (SeedTail); otherwise a launch of its own
    bool deferred;          // deferred exact evaluation: survivors appended with their bounds, resolved by launch_resolve
};
// rank_limits: a call under per-query probe depths (pqv_topk_depth) -- its one-query form goes through the general pair sort, which
// leaves the cut ranks out (the probe merge's own bucketing makes a quad of every rank)
static TopkRoute topk_route(const pqv_searcher *s, const TopkPlan &p, uint32_t nq, uint32_t k, bool rank_limits = false) {
    TopkRoute r{};
    r.screened = p.tile && p.filter && p.quad;
    if (!r.screened) return r;
    r.operand = p.i8 ? 2 : p.f16 ? 1 : 0;
    r.single_bucket = nq == 1 && p.np <= 64 && s->opt.single_bucket && !s->n_files && !rank_limits;
    r.fused_probe = r.single_bucket && s->opt.single_bucket > 0 && s->opt.single_bucket != 2 && s->kc_pad != 0 && s->kc_pad <= 4096;
    r.items = (s->opt.item_grid > 1 || (s->opt.item_grid == 1 && p.block_waves == 4)) &&
              static_cast<uint64_t>(p.max_quads) * p.filter_bpl <= (1ull << 24);
    r.max_items = r.items ? p.max_quads * p.filter_bpl : 0;
    r.wide = r.items && p.wide_width != 0 && !r.single_bucket;
    r.wide_max_items = r.wide ? p.max_quads * p.wide_bpl : 0;
    r.q_global = !p.f16 && !p.i8 && static_cast<uint64_t>(p.quad_width) * s->sdim * sizeof(float) > 32768;
    r.seed_tail = nq == 1 && k <= 256 && s->opt.single_bucket > 0;
    r.deferred = defer_route(s, nq, k, p);
    return r;
}

// A top-k call's device outputs, the optional ones nullptr where the caller takes none: rows and dist [nq, k * m] (m: rows per group,
// 1 off the grouped calls), n_found and n_cand [nq], group_key and group_rows [nq, k].  The host forms of the partition family
// carry the caller's HOST arrays in one too (PartitionHostOuts).
struct TopkOut {
    uint32_t *rows; float *dist; uint32_t *n_found; uint64_t *n_cand; int64_t *group_key; uint32_t *group_rows;
    // the block of the piece that starts at query q0 (km: k * m; the score form of the candidate-list calls, whose dist is indexed
    // by candidate, passes k = km = 0)
    TopkOut at(uint32_t q0, uint32_t k, size_t km) const {
        const size_t q = q0;
        return TopkOut{rows ? rows + q * km : nullptr, dist ? dist + q * km : nullptr, n_found ? n_found + q : nullptr,
                       n_cand ? n_cand + q : nullptr, group_key ? group_key + q * k : nullptr, group_rows ? group_rows + q * k : nullptr};
    }
};

// The two-pass fold of a distinct / grouped call (pqv.h: pqv_topk_grouped), probed (enqueue_topk) or over a key partition
// (enqueue_partition_grouped): n_part per-wave lists per query, group_size rows per group (0: a distinct call; 1: one row per group,
// its group_rows filled from n_found) of the k nearest groups of column col.  With more than one row per group, pass 1 is the distinct
// call with its rows and distances going to the lane, and pass 2 behind its fold fills the caller's [nq, k, group_size] blocks.
struct GroupFold {
    uint32_t k, group_size, n_part; const pqv_row_keys *col; int sqrt_out;
    bool two_pass() const { return group_size > 1; }
    size_t km() const { return static_cast<size_t>(k) * std::max<uint32_t>(1, group_size); }      // (64-bit: no wrap)
    bool fill(const TopkOut &o) const { return group_size == 1 && o.group_rows; }
    // Every buffer of both passes, for nq queries: called before the first kernel of the batch or piece (DevBuf::ensure may move a
    // buffer enqueued work still reads) -- the partial lists of pass 2 take over those of pass 1.  out: the caller's outputs.
    int size(Scratch &sc, uint32_t nq, const TopkOut &out) const {
        const size_t n_lists = static_cast<size_t>(nq) * n_part, km = this->km();
        HIP_TRY(sc.s_part_keys.ensure((n_lists * km + 4) * sizeof(uint64_t)));
        HIP_TRY(sc.s_part_vals.ensure((n_lists * km + 4) * sizeof(uint32_t)));
        HIP_TRY(sc.s_part_grp.ensure((n_lists * k + 4) * sizeof(int64_t)));
        if (two_pass()) {
            HIP_TRY(sc.s_gpart_slot.ensure((n_lists * km + 4) * sizeof(uint32_t)));
            HIP_TRY(sc.s_gpart_cnt.ensure((n_lists + 4) * sizeof(uint32_t)));
            HIP_TRY(sc.s_g1_rows.ensure(static_cast<size_t>(nq) * k * sizeof(uint32_t)));
            HIP_TRY(sc.s_g1_dist.ensure(static_cast<size_t>(nq) * k * sizeof(float)));
            HIP_TRY(sc.s_gset_keys.ensure(static_cast<size_t>(nq) * k * sizeof(int64_t)));
            HIP_TRY(sc.s_gset_slot.ensure(static_cast<size_t>(nq) * k * sizeof(uint32_t)));
            if (!out.group_key) HIP_TRY(sc.s_g1_keys.ensure(static_cast<size_t>(nq) * k * sizeof(int64_t)));
        }
        if ((two_pass() || fill(out)) && !out.n_found) HIP_TRY(sc.s_g1_nfound.ensure(static_cast<size_t>(nq) * sizeof(uint32_t)));
        return PQV_OK;
    }
    // o (a batch's or a piece's block) with what the caller does not take but the fold reads going to the lane: pass 1's group values
    // (read by the group set) and n_found (the group set, the rows-per-group fill).  The lane's buffers hold one batch or piece.
    TopkOut on_lane(Scratch &sc, TopkOut o) const {
        if (two_pass() && !o.group_key) o.group_key = sc.s_g1_keys.as<int64_t>();
        if ((two_pass() || fill(o)) && !o.n_found) o.n_found = sc.s_g1_nfound.as<uint32_t>();
        return o;
    }
    // The fold with at most one entry per group (distinct_merge_kernel) of the ra.nq queries' lists behind pass 1's walk, then a
    // grouped call's pass 2 -- the k groups as a sorted set per query, walk(ga) over their rows only, and the fold (no host step
    // between) -- or the rows-per-group fill.  s: the searcher whose rows are read; ra: pass 1's walk; out: on_lane's block.
    // walk gets GroupedArgs with the column, the set, the sizes and the partial lists filled, adds what only its path has and
    // launches its kernel.  Counted here: what is launched beyond the distinct merge.
    template <class Walk>
    int enqueue(const pqv_searcher *s, Scratch &sc, hipStream_t stream, const pqv::StreamArgs &ra, const TopkOut &out, Walk walk) const {
        using namespace pqv;
        const uint32_t nq = ra.nq, km = static_cast<uint32_t>(this->km());
        DistinctMergeArgs dm{};
        dm.part_keys = ra.part_keys; dm.part_vals = ra.part_vals; dm.part_grp = sc.s_part_grp.as<int64_t>();
        dm.nq = nq; dm.n_part = n_part; dm.k = k; dm.elem_size = col->elem_size();
        dm.ids = s->d_final_ids; dm.row_idx = two_pass() ? sc.s_g1_rows.as<uint32_t>() : out.rows;
        dm.dist = two_pass() ? sc.s_g1_dist.as<float>() : out.dist;
        dm.group_key = out.group_key; dm.n_found = out.n_found; dm.sqrt_out = sqrt_out;
        HIP_TRY(launch_distinct_merge(dm, stream));
        if (two_pass()) {
            HIP_TRY(launch_group_set(out.group_key, out.n_found, nq, k, sc.s_gset_keys.as<int64_t>(), sc.s_gset_slot.as<uint32_t>(), stream));
            GroupedArgs ga{};
            ga.key_pos = col->d_key_pos.p; ga.valid_pos = col->valid_image(); ga.elem_size = dm.elem_size;
            ga.set_keys = sc.s_gset_keys.as<int64_t>(); ga.set_slot = sc.s_gset_slot.as<uint32_t>(); ga.n_found = out.n_found;
            ga.k = k; ga.group_size = group_size; ga.km = km;
            ga.part_keys = sc.s_part_keys.as<uint64_t>(); ga.part_vals = sc.s_part_vals.as<uint32_t>();
            ga.part_slot = sc.s_gpart_slot.as<uint32_t>(); ga.part_cnt = sc.s_gpart_cnt.as<uint32_t>();
            if (int rc = walk(ga)) return rc;
            GroupedMergeArgs gma{};
            gma.part_keys = ga.part_keys; gma.part_vals = ga.part_vals; gma.part_slot = ga.part_slot; gma.part_cnt = ga.part_cnt;
            gma.nq = nq; gma.n_part = n_part; gma.k = k; gma.group_size = group_size; gma.km = km;
            gma.ids = s->d_final_ids; gma.row_idx = out.rows; gma.dist = out.dist; gma.group_rows = out.group_rows; gma.sqrt_out = sqrt_out;
            HIP_TRY(launch_grouped_merge(gma, stream));
            s->counters.kernel_launches += 3;
        } else if (fill(out)) {
            HIP_TRY(launch_group_rows_fill(out.n_found, nq, k, out.group_rows, stream));
            s->counters.kernel_launches += 1;
        }
        return PQV_OK;
    }
};

// One enqueue_topk call as its stages see it: the caller's arguments, the plan, route and request they follow, and what earlier
// stages leave for later ones.  Handed on by reference, never copied.
struct TopkCall {
    const pqv_searcher *s; Scratch &sc; hipStream_t stream;
    const TopkPlan &p; const TopkRoute &rt; const SearchRequest *rq;
    uint32_t nq, k, k_out, p0;                  // p0: an expanding call's own nprobe (the probe ranks p.np lists)
    uint64_t max_candidates, max_pos; int metric, sqrt_out;
    const float *d_queries, *d_queries_s;       // as given (the probe), and padded like the stored rows (pad_queries)
    uint32_t *d_row_idx; float *d_dist; uint32_t *d_n_found, *d_tie;
    hipEvent_t ev[4];
    pqv::MergeArgs pm;                          // the probe merge's arguments (probe_merge_args, enqueue_probe_stage)
    uint32_t *pair_u32;                         // tile paths: the pair sort's u32 scratch
    pqv::PairQuantArgs pq_args; bool quant_done;       // int8 screen: the query images' arguments; done inside the fused probe
    const uint64_t *pair_end;                   // round-robin capped table: every probed list's end of candidates
    const uint32_t *rank_limit;                 // expanding call: the lists each query walks (expand_depth)
    // a distinct / grouped call (group_buffers): its fold, and the outputs the fold writes (the caller's blocks, or the lane's)
    GroupFold gf; TopkOut g_out;
};
// stage: the probe works on the queries as given; everything that meets the (possibly zero-padded) stored rows gets the batch's
// queries padded the same way
static int pad_queries(TopkCall &c) {
    const pqv_searcher *s = c.s; Scratch &sc = c.sc;
    if (s->sdim == s->dim) return PQV_OK;
    HIP_TRY(sc.s_qpad.ensure(static_cast<size_t>(c.nq) * s->sdim * sizeof(float)));
    HIP_TRY(pqv::launch_pad_rows(c.d_queries, nullptr, c.nq, s->dim, s->sdim, sc.s_qpad.as<float>(), c.stream));
    c.d_queries_s = sc.s_qpad.as<float>();
    return PQV_OK;
}
// stage: the per-wave partial lists, and for a distinct / grouped call every buffer of both passes of its fold (GroupFold::size),
// before the first kernel
static int group_buffers(TopkCall &c) {
    Scratch &sc = c.sc; const TopkPlan &p = c.p; const SearchRequest *rq = c.rq;
    const uint32_t nq = c.nq, k = c.k;
    HIP_TRY(sc.s_part_keys.ensure((static_cast<size_t>(nq) * p.n_part_rr * k + 4) * sizeof(uint64_t)));
    HIP_TRY(sc.s_part_vals.ensure((static_cast<size_t>(nq) * p.n_part_rr * k + 4) * sizeof(uint32_t)));
    if (!rq || !rq->distinct()) return PQV_OK;
    c.gf = GroupFold{k, rq->groups.size, p.n_part_rr, rq->groups.col, c.sqrt_out};
    if (c.gf.two_pass() && (c.gf.km() > 1024 || k > pqv::GROUPED_SET_MAX)) return fail(PQV_ERR_INVALID, "grouped call beyond the kernels' lists");
    const TopkOut out{c.d_row_idx, c.d_dist, c.d_n_found, nullptr, rq->groups.d_keys, rq->groups.d_rows};
    if (int rc = c.gf.size(sc, nq, out)) return rc;
    c.g_out = c.gf.on_lane(sc, out);
    return PQV_OK;
}
// stage 1: the centroid probe with everything the probe merge presets or writes on the way -- the tile paths' histogram and empty
// partial lists, the one-query bucketing, and the int8 screen's query images (made inside the fused one-query probe)
static int enqueue_probe_stage(TopkCall &c, uint32_t nprobe) {
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const TopkPlan &p = c.p; const TopkRoute &rt = c.rt; hipStream_t stream = c.stream;
    const uint32_t nq = c.nq, k = c.k; const float *d_queries = c.d_queries, *d_queries_s = c.d_queries_s;
    pqv::MergeArgs &pm = c.pm; pqv::PairQuantArgs &pq_args = c.pq_args;
    const uint32_t kc_pairs = s->n_clusters;
    uint32_t *pair_u32 = nullptr, zero_n = 0;
    if (p.tile) {
        // u32 scratch: hist[R][kc] cursor[R][kc] pair_off[kc+1] group_off[kc+1] n_groups[1] quad_off[kc+1] n_quads[1]
        // (R = HIST_REPLICAS partial copies); the probe kernel zeroes hist, the probe merge fills it, the scan sets cursor
        constexpr uint64_t R = pqv::HIST_REPLICAS;
        HIP_TRY(sc.s_pair_u32.ensure(((2 * R + 5) * kc_pairs + 10) * sizeof(uint32_t)));      // + item_off[kc+1] n_items[1] wide_item_off[kc+1] wide_n_items[1]
        pair_u32 = sc.s_pair_u32.as<uint32_t>();
        zero_n = static_cast<uint32_t>(R * kc_pairs);
        HIP_TRY(sc.s_gthr.ensure(static_cast<size_t>(nq) * sizeof(unsigned long long)));
        if (p.filter) { HIP_TRY(sc.s_qnorm.ensure(static_cast<size_t>(nq) * sizeof(float))); HIP_TRY(sc.s_qmax.ensure(static_cast<size_t>(nq) * sizeof(float))); }
        pm.hist = pair_u32; pm.hist_stride = kc_pairs; pm.gthr_init = sc.s_gthr.as<unsigned long long>();
        // (per-query depths are decided behind the merge: probe_depth fills the histogram, below the limits)
        if (c.rq && c.rq->depth_only()) pm.hist = nullptr;
        // every partial list of the re-rank starts EMPTY: preset by the probe merge (one wave per query)
        if (rt.screened) {              // wide path: one "written" byte per list (see MergeArgs::preset_flags)
            const uint32_t nflag = (p.n_part_rr + 3) / 4 * 4;
            HIP_TRY(sc.s_part_flags.ensure(static_cast<size_t>(nq) * nflag));
            pm.preset_flags = sc.s_part_flags.as<uint8_t>(); pm.preset_flag_n = nflag;
        } else {
            pm.preset_keys = sc.s_part_keys.as<uint64_t>(); pm.preset_vals = sc.s_part_vals.as<uint32_t>();
            pm.preset_n = p.n_part_rr * k;
        }
        if (p.filter) { pm.qnorm_out = sc.s_qnorm.as<float>(); pm.qmax_out = sc.s_qmax.as<float>(); pm.queries = d_queries; pm.dim = s->dim; }
        HIP_TRY(sc.s_quads.ensure(static_cast<size_t>(p.max_quads) * sizeof(uint4)));
        HIP_TRY(sc.s_pairs.ensure(static_cast<size_t>(nq) * p.np * sizeof(uint32_t)));
        HIP_TRY(sc.s_groups.ensure(static_cast<size_t>(p.max_groups) * sizeof(uint4)));
        if (rt.items) HIP_TRY(sc.s_items.ensure(2 * (static_cast<size_t>(rt.max_items) + rt.wide_max_items) * sizeof(uint32_t)));
    }
    if (rt.single_bucket) {
        uint32_t *v = pair_u32 + 2 * (pqv::HIST_REPLICAS - 1) * static_cast<uint64_t>(kc_pairs);
        pm.sq_quads = sc.s_quads.as<uint4>(); pm.sq_pairs = sc.s_pairs.as<uint32_t>(); pm.sq_n_quads = v + 5ull * kc_pairs + 4;
        if (rt.items) {
            pm.sq_item_quad = sc.s_items.as<uint32_t>(); pm.sq_n_items = v + 6ull * kc_pairs + 6;
            pm.sq_item_rows = p.filter_rows_per_block; pm.sq_max_items = rt.max_items;
        }
    }
    // int8 screen: the query images (one per query, or one per probed pair in the residual form) -- see step 2
    if (rt.operand == 2) {
        if (int rc = ensure_blocked_copy(s, 2, stream)) return rc;     // centres and scales (built at creation; here only after an option change)
        const bool per_pair = s->i8_residual;
        const size_t n_img = per_pair ? static_cast<size_t>(nq) * p.np : nq;
        HIP_TRY(sc.s_qi8.ensure(n_img * s->sdim));
        HIP_TRY(sc.s_qn2i.ensure(n_img * sizeof(int)));
        HIP_TRY(sc.s_qres.ensure(n_img * sizeof(float)));
        HIP_TRY(sc.s_qresu.ensure(n_img * sizeof(float)));
        HIP_TRY(sc.s_pair_lb.ensure(n_img * sizeof(float)));
        pq_args = pqv::PairQuantArgs{d_queries_s, per_pair ? sc.s_probe.as<uint32_t>() : nullptr, s->d_center.as<float>(),
                                     s->d_list_scale.as<float>(), s->d_list_half.as<float>(), s->d_list_radius.as<float>(),
                                     static_cast<uint32_t>(n_img), per_pair ? p.np : 1u, s->sdim, static_cast<int8_t *>(sc.s_qi8.p),
                                     sc.s_qn2i.as<int>(), sc.s_qres.as<float>(), sc.s_qresu.as<float>(), sc.s_pair_lb.as<float>()};
    }
    if (c.rq && c.rq->depth_only() && c.rq->expand.source == DEPTH_RATIO) {     // the depth stage reads the ranks' probe distances
        HIP_TRY(sc.s_depth_d2.ensure(static_cast<size_t>(nq) * p.np * sizeof(uint32_t)));
        pm.probe_d2 = sc.s_depth_d2.as<uint32_t>();
    }
    if (rt.fused_probe) {
        pqv::ProbeRowsArgs pr{};
        pr.cent_t = s->d_cent_t.as<float4>(); pr.queries = d_queries;
        pr.nq = 1; pr.kc = s->n_clusters; pr.kc_pad = s->kc_pad; pr.dim = s->dim;
        HIP_TRY(sc.s_probe_keys.ensure(static_cast<size_t>(s->kc_pad) * sizeof(uint64_t)));
        pr.part_keys = sc.s_probe_keys.as<uint64_t>();
        if (!sc.s_ticket.p) {
            HIP_TRY(sc.s_ticket.ensure(sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(sc.s_ticket.p, 0, sizeof(uint32_t), stream));
        }
        // (the image(s) of a one-query call are made inside the probe launch)
        c.quant_done = pq_args.n_pairs != 0;
        HIP_TRY(pqv::launch_probe_single(pr, pm, sc.s_ticket.as<uint32_t>(), c.quant_done ? &pq_args : nullptr, stream));
    } else {
        if (int rc = enqueue_probe(s, sc, p, d_queries, nq, nprobe, c.max_candidates, pm, pair_u32, zero_n, stream, c.metric)) return rc;
    }
    c.pair_u32 = pair_u32;
    c.pair_end = table_rr(s, c.max_candidates) ? sc.s_pair_end.as<uint64_t>() : nullptr;   // (round-robin capped table)
    return PQV_OK;
}
// stage: an expanding call (pqv_topk_expand).  The probe ranked P = min(max_nprobe, n_clusters) lists per query; a counting pass and
// a select -- with a group column, one kernel over the distinct group values -- decide per query how many of them it walks
// (>= p0), and the stream pass runs under those rank limits (c.rank_limit).
static int expand_depth(TopkCall &c) {
    using namespace pqv;
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const TopkPlan &p = c.p; const SearchRequest *rq = c.rq; hipStream_t stream = c.stream;
    const uint32_t nq = c.nq, k_out = c.k_out, p0 = c.p0; const MergeArgs &pm = c.pm;
    uint32_t *used = rq->expand.d_used;
    if (!used) { HIP_TRY(sc.s_expand_used.ensure(static_cast<size_t>(nq) * sizeof(uint32_t))); used = sc.s_expand_used.as<uint32_t>(); }
    // (both forms before the stream pass: that pass adds n_cand[q] to candidate_rows)
    if (const pqv_row_keys *gk = rq->groups.col) {
        // a group column (pqv_topk_distinct_expand): DISTINCT group values in probe order, one block per query, one launch
        const GroupExpandArgs ga{sc.s_probe.as<uint32_t>(), sc.s_cand_base.as<uint64_t>(), s->d_list_off.as<uint64_t>(), nq, p.np, p0, k_out,
                                 rq->rows.bits, gk->d_key_pos.p, gk->valid_image(),
                                 gk->elem_size(), used, pm.n_cand};
        const GroupFilterArgs fa = rq->filtered() ? group_filter_args(rq) : GroupFilterArgs{};
        HIP_TRY(launch_group_expand(ga, rq->filtered() ? &fa : nullptr, stream));
        s->counters.kernel_launches += 1;
    } else {
        HIP_TRY(sc.s_expand_cnt.ensure(static_cast<size_t>(nq) * p.np * sizeof(uint32_t)));
        ExpandCountArgs ca{};
        ca.probe = sc.s_probe.as<uint32_t>(); ca.list_off = s->d_list_off.as<uint64_t>(); ca.nq = nq; ca.P = p.np;
        ca.bits = rq->rows.bits; ca.cnt = sc.s_expand_cnt.as<uint32_t>();
        if (const pqv_row_keys *kk = rq->rows.keys) {
            const uint32_t wide = kk->dtype == PQV_COL_I32 ? 0u : 1u;
            ca.win = 1u + 2u * rq->rows.kind + wide;
            ca.key_pos = kk->d_key_pos.p; ca.valid_pos = kk->valid_image();
            ca.a = rq->d_filter_a(); ca.b = rq->d_filter_b();
        }
        HIP_TRY(launch_filter_count(ca, stream));
        const ExpandSelectArgs sa{ca.cnt, ca.probe, sc.s_cand_base.as<uint64_t>(), ca.list_off, nq, p.np, p0, k_out, used, pm.n_cand};
        HIP_TRY(launch_expand_select(sa, stream));
        s->counters.kernel_launches += 2;
    }
    c.rank_limit = used;
    return PQV_OK;
}
// stage: a call with depths of its own (pqv_topk_depth).  The probe ranked P lists per query; one wave per query clamps the caller's
// depth, or counts the ranks within d2_ratio of the nearest centroid, into [p0, P].  Everything behind it runs under those limits:
// the pair sort leaves the cut pairs out (c.rank_limit), the kernels that walk by (query, rank) find no candidate in them
// (c.pair_end), and the candidate totals are those of the used lists -- counted here, the request's probe merge counts nothing.
static int probe_depth(TopkCall &c) {
    using namespace pqv;
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const SearchRequest *rq = c.rq;
    const uint32_t nq = c.nq, P = c.p.np;
    uint32_t *used = rq->expand.d_used;
    if (!used) { HIP_TRY(sc.s_expand_used.ensure(static_cast<size_t>(nq) * sizeof(uint32_t))); used = sc.s_expand_used.as<uint32_t>(); }
    HIP_TRY(sc.s_depth_end.ensure(static_cast<size_t>(nq) * P * sizeof(uint64_t)));
    const bool given = rq->expand.source == DEPTH_GIVEN;
    if (given && !rq->expand.d_depths) return fail(PQV_ERR_INVALID, "depths must not be NULL");
    const ProbeDepthArgs da{given ? rq->expand.d_depths : nullptr, given ? nullptr : c.pm.probe_d2, rq->expand.d2_ratio, sc.s_probe.as<uint32_t>(),
                            sc.s_cand_base.as<uint64_t>(), s->d_list_off.as<uint64_t>(), nq, P, c.p0, used, c.pm.n_cand,
                            sc.s_depth_end.as<uint64_t>(), s->d_stats.as<unsigned long long>(), c.p.tile ? c.pair_u32 : nullptr, s->n_clusters};
    HIP_TRY(launch_probe_depth(da, c.stream));
    s->counters.kernel_launches += 1;
    c.rank_limit = used;
    c.pair_end = sc.s_depth_end.as<uint64_t>();
    return PQV_OK;
}
// stage 2a: the probed (query, list) pairs bucketed by list into groups and quads (pair sort; one query: done by the probe merge),
// and the work-item tables of the wide screen.  ps: filled for the re-rank stages that read its tables.
static int enqueue_pair_sort(TopkCall &c, pqv::PairSortArgs &ps) {
    using namespace pqv;
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const TopkPlan &p = c.p; const TopkRoute &rt = c.rt; hipStream_t stream = c.stream;
    const uint32_t nq = c.nq;
    const uint32_t n_pairs = nq * p.np, kc = s->n_clusters;
    uint32_t *u = c.pair_u32;
    ps.probe = sc.s_probe.as<uint32_t>(); ps.n_pairs = n_pairs; ps.n_clusters = kc; ps.hist_done = 1;
    ps.rank_limit = c.rank_limit;          // (per-query depths: the histogram holds the pairs below them, see probe_depth)
    uint32_t *v = u + 2 * (pqv::HIST_REPLICAS - 1) * static_cast<uint64_t>(kc);    // past the extra histogram / cursor copies
    ps.hist = u; ps.hist_stride = kc; ps.nprobe = p.np; ps.cursor = u + pqv::HIST_REPLICAS * static_cast<uint64_t>(kc);
    ps.pair_off = v + 2ull * kc; ps.group_off = v + 3ull * kc + 1;
    ps.n_groups = v + 4ull * kc + 2;
    ps.quad_off = v + 4ull * kc + 3; ps.n_quads = v + 5ull * kc + 4; ps.quad_width = rt.wide ? p.wide_width : p.quad_width ? p.quad_width : 64;
    ps.pairs = sc.s_pairs.as<uint32_t>(); ps.groups = sc.s_groups.as<uint4>(); ps.quads = sc.s_quads.as<uint4>();
    // work items of the wide filter kernel (quad x row chunk that exists): its grid then has no holes
    // (the 8-wave blocks keep the 2-D grid with its quad-to-XCD affinity: C2 7.25 against 7.13 M QPS)
    if (rt.items) {
        ps.list_off = s->d_list_off.as<uint64_t>(); ps.item_rows = p.filter_rows_per_block;
        ps.item_off = v + 5ull * kc + 5; ps.n_items = v + 6ull * kc + 6;
        ps.item_quad = sc.s_items.as<uint32_t>(); ps.max_items = rt.max_items;
        if (s->opt.chunk_major && !rt.single_bucket) {
            ps.item_chunk = ps.item_quad + rt.max_items + rt.wide_max_items; ps.wide_item_chunk = ps.item_chunk + rt.max_items;
        }
        // the batch's shape for the NEXT batch's choice between the wide-quad instance and regular quads only (prefer_regular)
        const bool shape_hint = p.i8 && p.block_waves == 4 && p.quad_width == 96 && ps.item_chunk && s->opt.wide_quads == 1;
        if (((rt.wide && ps.item_chunk) || shape_hint) && !s->h_wide_stats.p) {
            HIP_TRY(s->h_wide_stats.ensure(4 * sizeof(uint32_t)));
            std::memset(s->h_wide_stats.p, 0, 4 * sizeof(uint32_t));
        }
        if (rt.wide && ps.item_chunk) ps.wide_stats = s->h_wide_stats.as<uint32_t>();    // pair_scan_kernel writes the two counts straight into pinned host memory
        if (shape_hint) { ps.shape_stats = s->h_wide_stats.as<uint32_t>() + 2; ps.shape_wide = 160; ps.shape_narrow = p.quad_width; }
        // XCD-aware slots: in the wide table always (lists of several wide quads); in the regular table where it has lists of
        // several quads too -- no wide-quad instance, or option 3 (every table)
        ps.xcd_items = !s->opt.xcd_items ? 0u : s->opt.xcd_items >= 3 ? 3u : rt.wide ? 2u : 1u;
        if (rt.wide) {
            ps.wide_list_major = p.list_once ? 1u : 0u;
            ps.wide_min = p.quad_width + 1; ps.wide_item_rows = p.wide_rows_per_block;
            ps.wide_item_off = v + 6ull * kc + 7; ps.wide_n_items = v + 7ull * kc + 8;
            ps.wide_item_quad = sc.s_items.as<uint32_t>() + rt.max_items; ps.wide_max_items = rt.wide_max_items;
        }
    }
    if (!rt.single_bucket) HIP_TRY(launch_pair_sort(ps, stream));
    return PQV_OK;
}
// stage 2b, the wide screen: upper bounds of the first seed_rows rows of every probed list (seed), the k-th smallest of them per query
// as the first threshold (select; one query: inside the seed launch), the screen over the whole lists with exact evaluation of what
// passes (filter), and -- deferred form -- the evaluation of the survivors left by their bounds (resolve)
static int enqueue_wide_screen(TopkCall &c, const pqv::PairSortArgs &ps, pqv::TileArgs &ta) {
    using namespace pqv;
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const TopkPlan &p = c.p; const TopkRoute &rt = c.rt; hipStream_t stream = c.stream;
    const uint32_t nq = c.nq, k = c.k; const float *d_queries_s = c.d_queries_s; const uint64_t max_pos = c.max_pos, *pair_end = c.pair_end;
    const uint32_t ccap = cand_cap_for(s, k);
    HIP_TRY(sc.s_cand_keys.ensure(static_cast<size_t>(nq) * ccap * sizeof(uint64_t)));
    HIP_TRY(sc.s_cand_vals.ensure(static_cast<size_t>(nq) * ccap * sizeof(uint32_t)));
    HIP_TRY(sc.s_cand_cnt.ensure(static_cast<size_t>(nq) * sizeof(uint32_t)));
    HIP_TRY(sc.s_spilled.ensure(static_cast<size_t>(nq) * sizeof(uint32_t)));
    ta.cand_keys = sc.s_cand_keys.as<uint64_t>(); ta.cand_vals = sc.s_cand_vals.as<uint32_t>();
    ta.cand_cnt = sc.s_cand_cnt.as<uint32_t>(); ta.cand_cap = ccap; ta.spilled = sc.s_spilled.as<uint32_t>();
    if (rt.deferred) {
        // deferred exact evaluation: bounds per appended pair, and the queues' raw scores (a strip per wave of every block)
        HIP_TRY(sc.s_cand_lb.ensure(static_cast<size_t>(nq) * ccap * sizeof(float)));
        const size_t blocks_r = rt.items ? rt.max_items : static_cast<size_t>(p.filter_bpl | 1u) * p.max_quads;
        const size_t words_r = blocks_r * p.block_waves * pqv::wide_filter_pend(p.quad_width, p.block_waves, p.f16);
        const size_t words_w = rt.wide ? static_cast<size_t>(rt.wide_max_items) * 8 * pqv::wide_filter_pend(p.wide_width, 8, false) : 0;
        HIP_TRY(sc.s_pendv.ensure((words_r + words_w) * sizeof(uint32_t)));
        ta.cand_lb = sc.s_cand_lb.as<float>();
        ta.pendv = sc.s_pendv.as<uint32_t>(); ta.pendv_wide = ta.pendv + words_r;
    }
    ta.static_dim = s->opt.static_dim ? 1u : 0u;       // (the seed kernel and the two filter instances)
    // thresholds: upper bounds of the first seed_rows rows of every probed list
    TileArgs seed = ta;
    if (rt.wide) seed.quad_width = p.wide_width;      // (the seed kernel samples a quad in slices of its own 64 queries)
    seed.row_offset = 0; seed.row_end = p.seed_rows; seed.rows_per_block = 256;
    seed.grid_x = (p.seed_rows + 255) / 256; seed.seed_sw = 4 * seed.grid_x;
    const uint32_t n_vals = p.np * seed.seed_sw * 16;
    HIP_TRY(sc.s_seed_ub.ensure(static_cast<size_t>(nq) * n_vals * sizeof(float)));
    seed.seed_ub = sc.s_seed_ub.as<float>();
    // (per-query depths: no quad holds a cut rank.  A batch's selection reads the bounds below the limits only; the one-query call
    //  selects inside the seed launch over all P ranks, so the cut ranks' bounds are preset to "none")
    if (c.rank_limit && rt.seed_tail) {
        HIP_TRY(launch_depth_seed_clear(seed.seed_ub, c.rank_limit, nq, p.np, seed.seed_sw * 16, stream));
        s->counters.kernel_launches += 1;
    }
    // running thresholds: see TileArgs::thr_hist
    if (s->opt.running_thr && k > 1) {
        HIP_TRY(sc.s_thr_hist.ensure(static_cast<size_t>(nq) * 16 * sizeof(uint32_t)));
        HIP_TRY(sc.s_thr_bins.ensure(static_cast<size_t>(nq) * sizeof(float4)));
        ta.thr_hist = sc.s_thr_hist.as<uint32_t>(); ta.thr_bins = static_cast<const float4 *>(sc.s_thr_bins.p);
    }
    pqv::SeedRefine rf{};
    if (seed_refine_on(s, nq, k)) {
        rf.mat = s->d_mat; rf.row_of = s->d_row_of; rf.queries = d_queries_s; rf.list_off = s->d_list_off.as<uint64_t>();
        rf.probe = sc.s_probe.as<uint32_t>(); rf.cand_base = sc.s_cand_base.as<uint64_t>();
        rf.dim = s->sdim; rf.nprobe = p.np; rf.seed_sw = seed.seed_sw; rf.seed_rows = p.seed_rows; rf.max_pos = max_pos;
        rf.pair_end = pair_end;
    }
    // one query: the seed kernel's last block selects (SeedTail); otherwise a launch of its own
    if (rt.seed_tail) {
        if (!sc.s_ticket2.p) {
            HIP_TRY(sc.s_ticket2.ensure(sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(sc.s_ticket2.p, 0, sizeof(uint32_t), stream));
        }
        seed.seed_tail.enable = 1; seed.seed_tail.n_vals = n_vals; seed.seed_tail.k = k;
        seed.seed_tail.gthr = ta.gthr; seed.seed_tail.cand_cnt = ta.cand_cnt; seed.seed_tail.spilled = ta.spilled;
        seed.seed_tail.thr_hist = ta.thr_hist; seed.seed_tail.thr_bins = static_cast<float4 *>(sc.s_thr_bins.p);
        seed.seed_tail.ticket = sc.s_ticket2.as<uint32_t>();
        seed.seed_tail.rf = rf;
    }
    HIP_TRY(launch_wide_seed(seed, stream));
    if (!rt.seed_tail)
        HIP_TRY(launch_seed_select(seed.seed_ub, nq, n_vals, k, ta.gthr, ta.cand_cnt, ta.spilled, stream,
                                   ta.thr_hist, static_cast<float4 *>(sc.s_thr_bins.p), &rf, c.rank_limit, seed.seed_sw * 16));
    ta.row_offset = 0; ta.slot_base = 0; ta.grid_x = p.filter_bpl;
    ta.rows_per_block = p.filter_rows_per_block; ta.filter_variant = 0;
    ta.part_flags = sc.s_part_flags.as<uint8_t>();
    if (rt.items) { ta.item_quad = ps.item_quad; ta.item_chunk = ps.item_chunk; ta.wide_item_chunk = ps.wide_item_chunk; ta.n_items = ps.n_items; ta.max_items = rt.max_items; }
    ta.drain_min = static_cast<uint32_t>(std::max(0, s->opt.drain_min)); // (whole-tile prefetch in the 96-query f16 form: 1000-row lists of 128 dims 5.96 -> 6.14 M q/s, C2's 10 k-row lists 7.68 -> 7.14 M)
    ta.opt_pf96 = (s->opt.pf96 >= 2 || (s->opt.pf96 == 1 && s->n / std::max<uint32_t>(1, s->n_clusters) <= 2048)) ? 1u : 0u;
    if (rt.wide) {
        ta.wide_width = p.wide_width; ta.wide_item_quad = ps.wide_item_quad; ta.wide_n_items = ps.wide_n_items;
        ta.wide_max_items = rt.wide_max_items; ta.wide_rows_per_block = p.wide_rows_per_block;
        ta.wide_nt = wide_rows_nt(s) ? 1u : 0u;
        ta.list_once = p.list_once ? 1u : 0u;
        if (s->opt.fork_wide) {
            if (!sc.side) {
                HIP_TRY(hipStreamCreateWithFlags(&sc.side, hipStreamNonBlocking));
                HIP_TRY(hipEventCreateWithFlags(&sc.ev_fork, hipEventDisableTiming));
                HIP_TRY(hipEventCreateWithFlags(&sc.ev_join, hipEventDisableTiming));
            }
            ta.side_stream = sc.side; ta.ev_fork = sc.ev_fork; ta.ev_join = sc.ev_join; ta.fork_wide_first = s->opt.fork_wide >= 2 ? 1u : 0u;
        }
        s->counters.kernel_launches += 1;
    }
    HIP_TRY(launch_tile_filter(ta, stream));
    s->counters.kernel_launches += 3;
    if (rt.deferred) {
        // the k-th smallest upper bound per query, then every band entry of the call on the whole chip (also for ONE query:
        // a single block evaluating K = 100 rows of 4 KB took 224 us inside the merge, 490 -> 390 us per call); the merge
        // then sees exact keys only.  (Part of the re-rank group: inside its timing events.)
        pqv::MergeArgs rm{};
        rm.nq = nq; rm.k = k; rm.cand_keys = ta.cand_keys; rm.cand_keys_rw = ta.cand_keys; rm.cand_vals = ta.cand_vals;
        rm.cand_cnt = ta.cand_cnt; rm.cand_cap = ccap; rm.cand_lb = ta.cand_lb;
        rm.mat = s->d_mat; rm.queries = d_queries_s; rm.dim = s->sdim; rm.resolve_stats = s->d_stats.as<unsigned long long>();
        // (one query, K = 100: the block evaluating its 100 defining rows alone is 50 of resolve_select's 81 us; the whole
        //  chip evaluates the 380-row band of the single cut in 13)
        rm.resolve_two_cuts = nq >= 32 ? 1 : 0;
        HIP_TRY(sc.s_work.ensure(static_cast<size_t>(nq) * ccap * sizeof(uint32_t) * 2));
        const bool counter_clean = sc.s_nwork.p != nullptr;       // (cleared by the previous call's final merge on this lane)
        HIP_TRY(sc.s_nwork.ensure(sizeof(uint32_t)));
        HIP_TRY(launch_resolve(rm, sc.s_work.p, sc.s_nwork.as<uint32_t>(), counter_clean, stream));
        s->counters.kernel_launches += 2;
    }
    return PQV_OK;
}
// stage 2b, the two older forms: the f32 tile filter behind an exact seed window, and the exact tile re-rank
static int enqueue_tile_forms(TopkCall &c, pqv::TileArgs &ta) {
    using namespace pqv;
    const pqv_searcher *s = c.s; const TopkPlan &p = c.p; hipStream_t stream = c.stream; const uint32_t nq = c.nq, k = c.k;
    if (p.filter) {
        TileArgs seed = ta;          // exact on rows [0, seed_rows) of every list: slot chunk 0
        seed.row_offset = 0; seed.slot_base = 0; seed.grid_x = 1; seed.row_end = p.seed_rows;
        seed.rows_per_block = std::max<uint32_t>(256, p.seed_rows);     // one 64-row tile per wave at least
        HIP_TRY(launch_tile_rerank(seed, stream));
        ta.row_offset = p.seed_rows; ta.slot_base = 4; ta.grid_x = p.filter_bpl;
        ta.rows_per_block = p.filter_rows_per_block; ta.filter_variant = 1;
        HIP_TRY(launch_seed_threshold(ta.part_keys, nq, p.np, p.slots_per_pair, k, ta.gthr, stream));
        HIP_TRY(launch_tile_filter(ta, stream));
        s->counters.kernel_launches += 2;
    } else {
        ta.row_offset = 0; ta.slot_base = 0; ta.grid_x = p.rr_bpl;
        HIP_TRY(launch_tile_rerank(ta, stream));
    }
    return PQV_OK;
}
// stage 2, the tile paths: the pair sort, the arguments every tile kernel shares, then the wide screen or one of the older forms
static int enqueue_tile_rerank(TopkCall &c) {
    using namespace pqv;
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const TopkPlan &p = c.p; const TopkRoute &rt = c.rt; hipStream_t stream = c.stream;
    const uint32_t nq = c.nq, k = c.k; const float *d_queries_s = c.d_queries_s; const uint64_t max_pos = c.max_pos, *pair_end = c.pair_end;
    const PairQuantArgs &pq_args = c.pq_args; hipEvent_t *ev = c.ev;
    PairSortArgs ps{};
    if (int rc = enqueue_pair_sort(c, ps)) return rc;
    TileArgs ta{};
    ta.mat = s->d_mat; ta.row_of = s->d_row_of; ta.list_off = s->d_list_off.as<uint64_t>();
    ta.queries = d_queries_s; ta.cand_base = sc.s_cand_base.as<uint64_t>();
    ta.pairs = ps.pairs; ta.groups = ps.groups; ta.n_groups = ps.n_groups; ta.max_groups = p.max_groups;
    ta.nq = nq; ta.nprobe = p.np; ta.dim = s->sdim; ta.k = k;
    ta.quads = ps.quads; ta.n_quads = ps.n_quads; ta.max_quads = p.max_quads; ta.quad_width = p.quad_width;
    ta.rows_per_block = p.rr_rows_per_block; ta.blocks_per_list = p.rr_bpl; ta.max_pos = max_pos; ta.pair_end = pair_end;
    ta.slots_per_pair = p.slots_per_pair; ta.slot_base = 0; ta.n_part = p.n_part_rr;
    ta.gthr = sc.s_gthr.as<unsigned long long>();
    ta.part_keys = sc.s_part_keys.as<uint64_t>(); ta.part_vals = sc.s_part_vals.as<uint32_t>();
    if (p.filter && !(p.quad && p.i8)) { if (int rc = ensure_row_norms(s, stream)) return rc; }    // (the f32 / f16 screens read the rows' norms)
    ta.row_norm2 = s->d_row_norm2.as<float>(); ta.norm_by_pos = s->images_only ? 1 : 0;
    ta.stats = s->d_stats.as<unsigned long long>();
    ta.xcd_swizzle = 0;
    if (rt.screened) {
        if (int rc = ensure_blocked_copy(s, rt.operand, stream)) return rc;     // built at creation; here only after an option change
        ta.mat_blk = static_cast<const float4 *>(s->d_mat_blk_op[rt.operand].p);
        ta.blk_off = s->d_blk_off.as<uint64_t>();
        ta.block_waves = p.block_waves;
        if (p.f16) {
            ta.f16 = 1; ta.scale = s->f16_scale; ta.scale2 = s->f16_scale * s->f16_scale;
            ta.query_maxabs = sc.s_qmax.as<float>();
        }
        if (p.i8) {
            // residual form: one image per (query, probed list) pair -- the query's residual against that list's centre at
            // that list's scale -- + the pair's lower bound from the triangle inequality on the centre (pair_lb);
            // one-centre form: one image per query (every list shares centre and scale)
            const bool per_pair = s->i8_residual;
            if (!c.quant_done) {
                HIP_TRY(launch_quantize_pairs_i8(pq_args.queries, pq_args.probe, pq_args.center, pq_args.scale, pq_args.half, pq_args.radius,
                                                 pq_args.n_pairs, pq_args.nprobe, pq_args.dim, pq_args.q_i8, pq_args.q_n2i, pq_args.q_res,
                                                 pq_args.q_resu, pq_args.pair_lb, stream, c.rank_limit));
                s->counters.kernel_launches += 1;
            }
            ta.i8 = 1; ta.i8_pair_images = per_pair ? 1 : 0;
            ta.q_i8 = static_cast<const int8_t *>(sc.s_qi8.p); ta.q_n2i = sc.s_qn2i.as<int>(); ta.q_res = sc.s_qres.as<float>();
            ta.q_resu = sc.s_qresu.as<float>(); ta.pair_lb = (per_pair && s->opt.pair_prune) ? sc.s_pair_lb.as<float>() : nullptr;
            ta.list_scale = s->d_list_scale.as<float>();
            ta.row_n2i = s->d_row_n2i.as<int>(); ta.row_res = s->d_row_res.as<float>();
        }
        // quad-to-XCD affinity: on by default for the global-query variant, whose per-quad operand copies
        // must stay L2-resident
        // (8-wave blocks: the quads of one cluster on one XCD, so a list's second pass finds rows in that L2: C3 2.51 -> 2.44 ms)
        ta.xcd_swizzle = s->opt.quad_xcd >= 0 ? s->opt.quad_xcd : (rt.q_global ? 1 : p.block_waves == 8 ? 2 : 0);
        if (rt.q_global) {
            // rows too long to stage a quad's queries in LDS: blocked copy per quad in global memory
            HIP_TRY(sc.s_qblk.ensure(static_cast<size_t>(p.max_quads) * p.quad_width * s->sdim * sizeof(float)));
            HIP_TRY(launch_pack_queries(d_queries_s, ps.pairs, ps.quads, ps.n_quads, p.max_quads, p.np, s->sdim,
                                        p.quad_width / 16, sc.s_qblk.p, stream));
            ta.q_blk = static_cast<const float4 *>(sc.s_qblk.p);
        }
    }
    if (p.filter) ta.query_norm2 = sc.s_qnorm.as<float>();     // filled by the probe merge
    if (ev[1]) HIP_TRY(hipEventRecord(ev[1], stream));
    if (int rc = rt.screened ? enqueue_wide_screen(c, ps, ta) : enqueue_tile_forms(c, ta)) return rc;
    if (ev[2]) HIP_TRY(hipEventRecord(ev[2], stream));
    s->counters.kernel_launches += 3;
    return PQV_OK;
}
// The arguments every candidate stream pass shares (top-k and range; after the probe: a capped table's pair ends are its output).  The
// caller adds its split (rows_per_block, blocks_per_list) and its outputs: the per-wave lists, or the range segments.
static pqv::StreamArgs stream_args(const pqv_searcher *s, Scratch &sc, const float *d_queries_s, uint32_t nq, uint32_t np, uint32_t k,
                                   uint64_t max_candidates, int metric) {
    pqv::StreamArgs ra{};
    ra.mat = s->d_mat; ra.row_of = s->d_row_of; ra.list_off = s->d_list_off.as<uint64_t>();
    ra.probe = sc.s_probe.as<uint32_t>(); ra.cand_base = sc.s_cand_base.as<uint64_t>();
    ra.queries = d_queries_s; ra.nq = nq; ra.nprobe = np; ra.dim = s->sdim; ra.k = k;
    ra.max_pos = max_candidates ? max_candidates : ~0ull; ra.metric = metric;
    ra.pair_end = table_rr(s, max_candidates) ? sc.s_pair_end.as<uint64_t>() : nullptr;   // (round-robin capped table)
    return ra;
}
// stage 3 of a distinct / grouped call: GroupFold's fold (no tie flag, k_out == k); pass 2 walks the probed lists again, under the
// call's row mask and per-query filter
static int enqueue_group_fold(TopkCall &c, const pqv::StreamArgs &ra) {
    using namespace pqv;
    const pqv_searcher *s = c.s; const SearchRequest *rq = c.rq; hipStream_t stream = c.stream;
    if (c.p.tile || c.k_out != c.k || c.d_tie) return fail(PQV_ERR_INVALID, "distinct call on a non-distinct plan");
    return c.gf.enqueue(s, c.sc, stream, ra, c.g_out, [&](GroupedArgs &ga) {
        ga.bits = rq->rows.bits; ga.stats = s->d_stats.as<unsigned long long>();
        ga.rank_limit = c.rank_limit;      // (an expanding call: both passes walk the same ranks)
        if (rq->filtered()) HIP_TRY(launch_grouped_filter_stream(ra, ga, group_filter_args(rq), stream));
        else HIP_TRY(launch_grouped_stream(ra, ga, stream));
        return static_cast<int>(PQV_OK);
    });
}
// stage 3 of every other call: the final merge of the per-wave lists (and the wide screen's candidate buffers)
static int enqueue_plain_fold(TopkCall &c, const pqv::StreamArgs &ra) {
    using namespace pqv;
    const pqv_searcher *s = c.s; Scratch &sc = c.sc; const TopkPlan &p = c.p; const TopkRoute &rt = c.rt; hipStream_t stream = c.stream;
    const uint32_t nq = c.nq, k = c.k;
    MergeArgs fm{};
    fm.part_keys = ra.part_keys; fm.part_vals = ra.part_vals;
    fm.nq = nq; fm.n_part = p.n_part_rr; fm.k_part = k; fm.k = k;
    fm.ids = s->d_final_ids; fm.row_idx = c.d_row_idx; fm.dist = c.d_dist; fm.n_found = c.d_n_found;
    fm.sqrt_out = c.sqrt_out; fm.k_out = c.k_out; fm.tie_flag = c.d_tie;
    if (rt.screened) {        // wide screened path: the final merge also reads the candidate buffers
        fm.cand_keys = sc.s_cand_keys.as<uint64_t>(); fm.cand_vals = sc.s_cand_vals.as<uint32_t>();
        fm.cand_cnt = sc.s_cand_cnt.as<uint32_t>(); fm.cand_cap = cand_cap_for(s, k);
        fm.spilled = sc.s_spilled.as<uint32_t>();
        fm.part_flags = sc.s_part_flags.as<uint8_t>();       // row stride: (n_part + 3) / 4 * 4 == n_part (a multiple of 4 waves)
    }
    if (rt.deferred) fm.zero_after = sc.s_nwork.as<uint32_t>();
    if (c.metric == PQV_DOT) {     // (keys carry ord(dist): dot_merge_kernel undoes it; no tie flags to raise)
        if (p.tile) return fail(PQV_ERR_INVALID, "PQV_DOT call on a screened plan");
        HIP_TRY(launch_dot_merge(fm, stream));
    } else
    HIP_TRY(launch_merge_final(fm, stream));
    return PQV_OK;
}

// Enqueue probe -> probe-merge -> re-rank -> final merge for one batch on `stream`: the stages above, in order.
// `k` is the list length the kernels work with; the first k_out entries are written out.
// With k == k_out + 1 the merge can also flag queries whose output distances tie (d_tie).
// Every buffer of both passes of a grouped call is sized (group_buffers) before the first kernel behind the query padding.
int enqueue_topk(const pqv_searcher *s, const float *d_queries, uint32_t nq, uint32_t k,
                 uint32_t k_out, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                 uint32_t *d_row_idx, float *d_dist, uint32_t *d_n_found, uint64_t *d_n_cand,
                 uint32_t *d_tie, hipStream_t stream, Scratch &sc, const SearchRequest *rq = nullptr) {
    using namespace pqv;
    // an expanding call (pqv_topk_expand): the probe ranks P = min(max_nprobe, n_clusters) lists per query (expand_depth)
    // a call with depths of its own (pqv_topk_depth) keeps the plain call's plan for P lists (probe_depth)
    const bool expand = rq && rq->expanding(), distinct = rq && rq->distinct(), depth = rq && rq->depth_only();
    const uint32_t p0 = probe_count(s, nprobe);
    nprobe = probe_arg(rq, nprobe);
    const TopkPlan p = plan_topk(s, nq, nprobe, k, metric, stream_request(rq));
    if (depth && (distinct || rq->filtered() || rq->rows.bits)) return fail(PQV_ERR_INVALID, "a depth call takes no filter and no grouping");
    if (expand && (s->n_files || (p.tile && !depth) || metric == PQV_DOT || max_candidates || p0 == 0 || p0 > p.np))
        return fail(PQV_ERR_INVALID, "expanding call on a plan that cannot expand");
    const TopkRoute rt = topk_route(s, p, nq, k, depth);
    TopkCall c{s, sc, stream, p, rt, rq, nq, k, k_out, p0, max_candidates, max_candidates ? max_candidates : ~0ull, metric, sqrt_out,
               d_queries, d_queries, d_row_idx, d_dist, d_n_found, d_tie};
    if (int rc = pad_queries(c)) return rc;

    // 1. centroid probe (its scratch first: the arguments below point into it)
    if (int rc = probe_merge_args(s, sc, p, nq, max_candidates, c.pm)) return rc;
    if (d_n_cand) c.pm.n_cand = d_n_cand;
    // (a request: candidate_rows and embeddings_fetched -- the considered rows -- are counted by the stream kernel)
    c.pm.stats = rq ? nullptr : s->d_stats.as<unsigned long long>();
    if (int rc = group_buffers(c)) return rc;
    if (int rc = timing_events(s, c.ev)) return rc;
    if (c.ev[0]) HIP_TRY(hipEventRecord(c.ev[0], stream));
    if (int rc = enqueue_probe_stage(c, nprobe)) return rc;
    if (expand) { if (int rc = depth ? probe_depth(c) : expand_depth(c)) return rc; }

    // 2. candidate re-rank + per-wave top-k
    if (p.tile) { if (int rc = enqueue_tile_rerank(c)) return rc; }
    StreamArgs ra = stream_args(s, sc, c.d_queries_s, nq, p.np, k, max_candidates, metric);
    ra.rows_per_block = p.rr_rows_per_block; ra.blocks_per_list = p.rr_bpl;
    ra.part_keys = sc.s_part_keys.as<uint64_t>(); ra.part_vals = sc.s_part_vals.as<uint32_t>();
    if (!p.tile) {
        if (c.ev[1]) HIP_TRY(hipEventRecord(c.ev[1], stream));
        if (depth) {       // (no filter: the plain walk, a cut rank's blocks storing empty lists; probe_depth has counted the candidates)
            HIP_TRY(launch_limited_stream(ra, MaskedArgs{nullptr, nullptr, nullptr, c.rank_limit}, stream));
        } else
        HIP_TRY(launch_stream_pass(ra, rq, s->d_stats.as<unsigned long long>(), c.pm.n_cand, STREAM_TOPK, stream,
                                   distinct ? sc.s_part_grp.as<int64_t>() : nullptr, c.rank_limit));
        if (c.ev[2]) HIP_TRY(hipEventRecord(c.ev[2], stream));
    }

    // 3. fold the per-wave lists, and the epilogue
    if (int rc = distinct ? enqueue_group_fold(c, ra) : enqueue_plain_fold(c, ra)) return rc;
    if (c.ev[3]) HIP_TRY(hipEventRecord(c.ev[3], stream));
    s->counters.kernel_launches += 4;
    return PQV_OK;
}

int validate_topk(const pqv_searcher *s, uint32_t k, uint32_t nprobe, int metric) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");                         // search.rs:67
    if (nprobe == 0) return fail(PQV_ERR_INVALID, "nprobe must be > 0");               // search.rs:72
    if (metric != PQV_L2SQ_REF4 && metric != PQV_L2SQ_SEQ && metric != PQV_COSINE && metric != PQV_DOT) return fail(PQV_ERR_INVALID, "unknown metric");
    return PQV_OK;
}
// ... and of the entry points that take queries from the host (pqv_topk, pqv_range_search with k = 1, pqv_probe with k = 1 and
// PQV_L2SQ_REF4: neither takes a k, pqv_probe no metric)
int validate_query(const pqv_searcher *s, uint32_t k, uint32_t nprobe, int metric, uint64_t max_candidates, uint32_t query_len) {
    if (int rc = validate_topk(s, k, nprobe, metric)) return rc;
    if (int rc = table_max_candidates(s, max_candidates)) return rc;
    if (query_len != s->dim)                                                           // search.rs:91-98
        return fail(PQV_ERR_INVALID, "Query dimension mismatch: expected " + std::to_string(s->dim) +
                                         ", got " + std::to_string(query_len));
    return PQV_OK;
}
// the kernels' sorted lists hold up to 1024 entries (k, and the probe's min(nprobe, n_clusters)); pqv_topk goes around
// that limit (topk_unbounded), the asynchronous device entry points report it
bool beyond_kernel_lists(const pqv_searcher *s, uint32_t k_lists, uint32_t nprobe) {
    return k_lists > 1024 || probe_count(s, nprobe) > 1024;
}
// a grouped call's lists hold k * group_size entries (64-bit: no wrap)
bool grouped_beyond_kernel_lists(const pqv_searcher *s, uint32_t k, uint32_t group_size, uint32_t nprobe) {
    return static_cast<uint64_t>(k) * group_size > 1024 || probe_count(s, nprobe) > 1024;
}
// PQV_DOT (pqv.h): every entry point works within the kernels' lists, and keyed / distinct calls do not take it.  Checked behind
// validate_topk, before any device work.
int dot_checks(const pqv_searcher *s, uint32_t k, uint32_t nprobe, int metric, const SearchRequest *rq) {
    if (metric != PQV_DOT) return PQV_OK;
    if (rq && (rq->filtered() || rq->distinct())) return fail(PQV_ERR_UNSUPPORTED, "PQV_DOT is not supported by keyed and distinct calls");
    if (beyond_kernel_lists(s, k, nprobe)) return fail(PQV_ERR_UNSUPPORTED, "PQV_DOT takes k <= 1024 and at most 1024 probed lists per query");
    return PQV_OK;
}

}  // namespace

namespace {

// ---- exact replay of the reference's heap for one query ----------------------------------
// std::collections::BinaryHeap<HeapItem> as src/ivf/search.rs:113-127 / exec.rs:264,474-481
// drive it (max-heap on distance; Ord = partial_cmp().unwrap_or(Equal)), restated from the
// published std source: push = append + sift_up (stops on <=), pop = swap_remove(0) +
// sift_down_to_bottom (right child on ties) + sift_up.  Only used for queries whose output
// distances tie, where survivors and order depend on this exact mechanics.
struct HeapEnt { float d; uint32_t row; };

inline bool ent_le(const HeapEnt &a, const HeapEnt &b) { return !(a.d > b.d); }

inline void heap_sift_up(std::vector<HeapEnt> &h, size_t start, size_t pos) {
    const HeapEnt e = h[pos];
    while (pos > start) {
        const size_t parent = (pos - 1) / 2;
        if (ent_le(e, h[parent])) break;
        h[pos] = h[parent];
        pos = parent;
    }
    h[pos] = e;
}

inline void heap_push(std::vector<HeapEnt> &h, HeapEnt e) {
    h.push_back(e);
    heap_sift_up(h, 0, h.size() - 1);
}

inline void heap_pop(std::vector<HeapEnt> &h) {
    HeapEnt item = h.back();
    h.pop_back();
    if (h.empty()) return;
    std::swap(item, h[0]);
    const size_t end = h.size();
    size_t pos = 0;
    const HeapEnt e = h[0];
    size_t child = 1;
    while (end >= 2 && child <= end - 2) {
        if (ent_le(h[child], h[child + 1])) child += 1;
        h[pos] = h[child];
        pos = child;
        child = 2 * pos + 1;
    }
    if (child == end - 1) { h[pos] = h[child]; pos = child; }
    h[pos] = e;
    heap_sift_up(h, 0, pos);
}

// Recompute one query's candidate distances on the device (STREAM_DIST), then replay them
// through the heap in candidate order.  d_probe / d_cand_base: the query's probe list on the device; `clusters` the
// same list on the host.  Any k (the selection is the heap's), any nprobe (the grid is cut into slices of probed lists).
// A round-robin capped table (table_rr) replays each list up to its file's quota (table_pair_ends; `nprobe` is read there only).
// allow (a masked or keyed call: its RowFilter): a capped candidate whose row does not pass is skipped in arrival order -- it never
// meets the heap; *considered = the rows that did.
int replay_with_clusters(const pqv_searcher *s, Scratch &sc, const float *d_query, const uint32_t *d_probe,
                         const uint64_t *d_cand_base, const std::vector<uint32_t> &clusters, uint32_t k,
                         uint64_t max_candidates, int metric, int sqrt_out, uint32_t *row_idx, float *dist,
                         uint32_t *n_found, uint32_t nprobe = 0, const RowFilter *allow = nullptr, uint64_t *considered = nullptr) {
    using namespace pqv;
    const uint32_t np = static_cast<uint32_t>(clusters.size());
    uint64_t total = 0;
    for (uint32_t c : clusters) total += s->h_list_off[c + 1] - s->h_list_off[c];
    const uint64_t use = max_candidates ? std::min<uint64_t>(total, max_candidates) : total;
    std::vector<float> d(std::max<uint64_t>(1, total));
    if (total) {
        HIP_TRY(sc.s_replay.ensure(total * sizeof(float)));
        for (uint32_t j0 = 0; j0 < np; j0 += 32768) {                   // gridDim.y <= 65535
            StreamArgs ra{};
            ra.mat = s->d_mat; ra.row_of = s->d_row_of; ra.list_off = s->d_list_off.as<uint64_t>();
            ra.probe = d_probe + j0; ra.cand_base = d_cand_base + j0;
            ra.queries = d_query; ra.nq = 1; ra.nprobe = std::min<uint32_t>(32768, np - j0); ra.dim = s->sdim; ra.k = 1;     // d_query: sdim wide
            ra.rows_per_block = 1024;
            ra.blocks_per_list = static_cast<uint32_t>((std::max<uint64_t>(1, s->max_list_len) + 1023) / 1024);
            ra.max_pos = ~0ull; ra.metric = metric; ra.out_f32 = sc.s_replay.as<float>();
            HIP_TRY(launch_stream(ra, STREAM_DIST, s->stream));
            s->counters.kernel_launches += 1;
        }
        HIP_TRY(hipMemcpyAsync(d.data(), sc.s_replay.p, total * sizeof(float), hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
    }
    std::vector<HeapEnt> heap;
    heap.reserve(static_cast<size_t>(std::min<uint64_t>(k, use)) + 1);
    std::vector<uint64_t> pair_end;
    if (table_rr(s, max_candidates)) table_pair_ends(s, clusters, nprobe, max_candidates, pair_end);
    uint64_t base = 0, n_considered = 0;
    const std::vector<uint32_t> *h_rows = s->h_rows->get();             // (the index' host lists: downloaded by the first call that reads them)
    if (!h_rows) return PQV_ERR_HIP;
    for (size_t j = 0; j < clusters.size(); ++j) {                      // candidate_rows order
        const uint32_t c = clusters[j];
        const uint64_t b = s->h_list_off[c], e = s->h_list_off[c + 1], lim = pair_end.empty() ? use : pair_end[j];
        uint64_t pos = base;
        base += e - b;
        for (uint64_t i = b; i < e && pos < lim; ++i, ++pos) {
            const HeapEnt ent{d[pos], (*h_rows)[i]};
            if (allow && !allow->pass(ent.row)) continue;
            ++n_considered;
            if (heap.size() < k) heap_push(heap, ent);                   // search.rs:119-120
            else if (ent.d < heap[0].d) { heap_pop(heap); heap_push(heap, ent); }   // :121-125
        }
    }
    if (sqrt_out == 1) for (auto &h : heap) h.d = std::sqrt(h.d);        // :133 (IEEE sqrtf)
    std::stable_sort(heap.begin(), heap.end(), [](const HeapEnt &a, const HeapEnt &b) { return a.d < b.d; });
    if (sqrt_out == 2) for (auto &h : heap) h.d = 0.5f * h.d;            // PQV_COSINE: sorted on d2, halved on the way out
    for (uint32_t i = 0; i < k; ++i) {
        if (i < heap.size()) { row_idx[i] = heap[i].row; dist[i] = heap[i].d; }
        else { row_idx[i] = 0xFFFFFFFFu; dist[i] = INFINITY; }
    }
    if (n_found) *n_found = static_cast<uint32_t>(heap.size());
    if (considered) *considered = n_considered;
    return PQV_OK;
}

// qi indexes the current sub-batch's probe scratch (written by the probe merge).
int replay_query_exact(const pqv_searcher *s, Scratch &sc, const float *d_query, uint32_t qi, uint32_t np, uint32_t k,
                       uint64_t max_candidates, int metric, int sqrt_out, uint32_t *row_idx, float *dist,
                       uint32_t *n_found, uint32_t nprobe, const RowFilter *allow = nullptr, uint32_t stride = 0) {
    // (stride: the probe table's lists per query where the replay takes the first np of them only -- an expanding call)
    if (!stride) stride = np;
    std::vector<uint32_t> clusters(np);
    HIP_TRY(hipMemcpyAsync(clusters.data(), sc.s_probe.as<uint32_t>() + static_cast<size_t>(qi) * stride,
                           np * sizeof(uint32_t), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    return replay_with_clusters(s, sc, d_query, sc.s_probe.as<uint32_t>() + static_cast<size_t>(qi) * stride,
                                sc.s_cand_base.as<uint64_t>() + static_cast<size_t>(qi) * stride, clusters, k, max_candidates,
                                metric, sqrt_out, row_idx, dist, n_found, nprobe, allow);
}

// find_closest_centroids (index.rs:130-149) without the kernels' list limit: every centroid distance on the GPU
// (STREAM_DIST over the centroid table), the stable sort on the host.  d_query: device [dim]; order: all clusters, nearest first.
// (a table searcher: the probed lists only -- see below; `nprobe` is read on tables only)
int centroid_order_host(const pqv_searcher *s, Scratch &sc, const float *d_query, std::vector<uint32_t> &order, uint32_t nprobe) {
    using namespace pqv;
    const uint32_t kc = s->n_clusters;
    HIP_TRY(sc.s_replay.ensure(std::max<size_t>(1, kc) * sizeof(float)));
    std::vector<float> cd(kc);
    StreamArgs pa{};
    pa.mat = s->d_centroids.as<float>(); pa.row_of = nullptr; pa.list_off = nullptr; pa.probe = nullptr; pa.cand_base = nullptr;
    pa.single_begin = 0; pa.single_end = kc;
    pa.queries = d_query; pa.nq = 1; pa.nprobe = 1; pa.dim = s->dim; pa.k = 1;
    pa.rows_per_block = 256; pa.blocks_per_list = (kc + 255) / 256;
    pa.max_pos = ~0ull; pa.metric = PQV_L2SQ_REF4;        // find_closest_centroids always uses index.rs:461
    pa.out_f32 = sc.s_replay.as<float>();
    HIP_TRY(launch_stream(pa, STREAM_DIST, s->stream));
    HIP_TRY(hipMemcpyAsync(cd.data(), sc.s_replay.p, static_cast<size_t>(kc) * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    order.resize(kc);
    for (uint32_t c = 0; c < kc; ++c) order[c] = c;
    if (!s->n_files) {
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return cd[a] < cd[b]; });   // index.rs:143-147
    } else {
        // a table: each file's centroids in their own order, file after file, and only the first nprobe of each are probed --
        // order becomes the probed lists, P = probe_count(s, nprobe) of them
        uint32_t o = 0;
        for (uint32_t f = 0; f < s->n_files; ++f) {
            const uint32_t lo = s->seg_off[f], hi = s->seg_off[f + 1], kf = std::min<uint32_t>(nprobe, hi - lo);
            std::stable_sort(order.begin() + lo, order.begin() + hi, [&](uint32_t a, uint32_t b) { return cd[a] < cd[b]; });
            std::copy(order.begin() + lo, order.begin() + lo + kf, order.begin() + o);
            o += kf;
        }
        order.resize(o);
    }
    s->counters.kernel_launches += 1;
    return PQV_OK;
}

// The centroid probe on the host (P > 1024; topk_unbounded): per query (device, dim wide) centroid_order_host -> its P probed lists
// in clusters [nq * P], its candidate total in totals[q].  With `upload` also what enqueue_probe leaves: sc.s_probe / s_cand_base
// and, on a round-robin capped table (table_rr), sc.s_pair_end (table_pair_ends).
int host_probe(const pqv_searcher *s, Scratch &sc, const float *d_queries, uint32_t nq, uint32_t nprobe, uint64_t max_candidates,
               bool upload, std::vector<uint32_t> &clusters, uint64_t *totals) {
    const uint32_t np = probe_count(s, nprobe);
    const size_t n = static_cast<size_t>(nq) * np;
    const bool rr = upload && table_rr(s, max_candidates);
    std::vector<uint32_t> order;
    std::vector<uint64_t> base(upload ? n : 0), end(rr ? n : 0), end_q;
    clusters.resize(n);
    for (uint32_t q = 0; q < nq; ++q) {
        if (int rc = centroid_order_host(s, sc, d_queries + static_cast<uint64_t>(q) * s->dim, order, nprobe)) return rc;
        order.resize(np);
        uint64_t total = 0;
        for (uint32_t j = 0; j < np; ++j) {
            clusters[static_cast<size_t>(q) * np + j] = order[j];
            if (upload) base[static_cast<size_t>(q) * np + j] = total;
            total += s->h_list_off[order[j] + 1] - s->h_list_off[order[j]];
        }
        if (rr) {
            table_pair_ends(s, order, nprobe, max_candidates, end_q);
            std::copy(end_q.begin(), end_q.end(), end.begin() + static_cast<size_t>(q) * np);
        }
        totals[q] = total;
    }
    if (!upload) return PQV_OK;
    if (int rc = ensure_probe_slots(s, sc, nq, np)) return rc;
    HIP_TRY(hipMemcpyAsync(sc.s_probe.p, clusters.data(), n * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(sc.s_cand_base.p, base.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    if (rr) {
        HIP_TRY(sc.s_pair_end.ensure(n * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(sc.s_pair_end.p, end.data(), n * sizeof(uint64_t), hipMemcpyHostToDevice, s->stream));
    }
    return PQV_OK;
}

// topk() beyond the kernels' list capacity (k >= 1024: no runner-up slot left; min(nprobe, n_clusters) > 1024): the
// reference accepts any NonZeroUsize (search.rs:56-81).  Per query: host_probe, every
// candidate distance on the GPU, the reference's heap on the host.  Correct for any k / nprobe; not a fast path.
int topk_unbounded(const pqv_searcher *s, Scratch &sc, const float *queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                   uint64_t max_candidates, int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found,
                   uint64_t *n_candidates, const SearchRequest *rq = nullptr) {
    using namespace pqv;
    HIP_TRY(sc.s_queries.ensure(static_cast<size_t>(s->dim) * sizeof(float)));
    std::vector<uint32_t> clusters;
    RowFilter allow;
    for (uint32_t q = 0; q < nq; ++q) {
        if (int rc = row_filter(s, rq, q, allow)) return rc;
        HIP_TRY(hipMemcpyAsync(sc.s_queries.p, queries + static_cast<uint64_t>(q) * s->dim, static_cast<size_t>(s->dim) * sizeof(float),
                               hipMemcpyHostToDevice, s->stream));
        uint64_t total = 0;
        // (no pair ends: the replay applies a table's round-robin cap on the host)
        if (int rc = host_probe(s, sc, sc.s_queries.as<float>(), 1, nprobe, 0, true, clusters, &total)) return rc;
        const float *d_q_s = sc.s_queries.as<float>();
        if (s->sdim != s->dim) {
            HIP_TRY(sc.s_qpad.ensure(static_cast<size_t>(s->sdim) * sizeof(float)));
            HIP_TRY(launch_pad_rows(sc.s_queries.as<float>(), nullptr, 1, s->dim, s->sdim, sc.s_qpad.as<float>(), s->stream));
            d_q_s = sc.s_qpad.as<float>();
        }
        uint32_t nf = 0;
        uint64_t considered = 0;
        if (int rc = replay_with_clusters(s, sc, d_q_s, sc.s_probe.as<uint32_t>(), sc.s_cand_base.as<uint64_t>(),
                                          clusters, k, max_candidates, metric, sqrt_out, row_idx + static_cast<uint64_t>(q) * k,
                                          dist + static_cast<uint64_t>(q) * k, &nf, nprobe, allow.active() ? &allow : nullptr, &considered))
            return rc;
        if (n_found) n_found[q] = nf;
        if (n_candidates) n_candidates[q] = total;
        s->counters.candidate_rows += total;                             // index_exec.rs:289-299
        s->counters.embeddings_fetched += considered;                    // exec.rs:411-427 (unmasked: min(total, max_candidates))
        s->counters.queries += 1;
        s->counters.exact_replays += 1;
    }
    return PQV_OK;
}

}  // namespace

// The host entry points' PQV_COSINE queries: the cosine layout (ensure_cosine), then n(q) of host queries [nq, dim] computed on the device
// (one normalize_rows_kernel launch on the searcher's stream) and brought back into `out`; then the call's arguments are pointed at
// the cosine searcher's own L2 search over them, its write-out halving d2 (sqrt_out 2).  Any other metric: nothing happens.
static int cosine_queries_host(const pqv_searcher *&s, const float *&queries, uint32_t nq, int &metric, int &sqrt_out, std::vector<float> &out) {
    if (metric != PQV_COSINE) return PQV_OK;
    std::lock_guard<std::mutex> lock(s->mu);
    if (int rc = ensure_cosine(s)) return rc;
    const size_t n = static_cast<size_t>(nq) * s->dim;
    try { out.resize(n); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
    Lane lane;
    if (int rc = lane.acquire(s, s->stream)) return rc;
    HIP_TRY(lane->s_queries.ensure(n * sizeof(float)));
    HIP_TRY(lane->s_qcos.ensure(n * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(lane->s_queries.p, queries, n * sizeof(float), hipMemcpyHostToDevice, s->stream));
    HIP_TRY(pqv::launch_normalize_rows(lane->s_queries.as<float>(), s->dim, nullptr, nq, s->dim, lane->s_qcos.as<float>(), s->stream));
    HIP_TRY(hipMemcpyAsync(out.data(), lane->s_qcos.p, n * sizeof(float), hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (int rc = lane.release()) return rc;
    queries = out.data(); s = s->cos.get(); metric = PQV_L2SQ_REF4; sqrt_out = 2;
    return PQV_OK;
}
// The device entry points' PQV_COSINE queries: the cosine layout, then n(q) of the device queries into `lane` -- THIS searcher's, taken
// here on the caller's stream -- as s_qcos.  The caller runs the cosine searcher's L2 body on the same stream (sqrt_out 2) and
// releases the lane behind it: its `done` event follows that call's kernels.
static int cosine_queries_device(const pqv_searcher *s, const float *d_queries, uint32_t nq, hipStream_t stream, Lane &lane) {
    if (int rc = ensure_cosine(s)) return rc;
    if (int rc = lane.acquire(s, stream)) return rc;
    HIP_TRY(lane->s_qcos.ensure(static_cast<size_t>(nq) * s->dim * sizeof(float)));
    HIP_TRY(pqv::launch_normalize_rows(d_queries, s->dim, nullptr, nq, s->dim, lane->s_qcos.as<float>(), stream));
    return PQV_OK;
}

static int pqv_topk_device_impl(const pqv_searcher *s, const void *d_queries, uint32_t nq, uint32_t k,
                               uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                               void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                               void *d_tie_flags, void *hip_stream, const SearchRequest *rq = nullptr) {
    if (int rc = validate_topk(s, k, nprobe, metric)) return rc;
    if (int rc = dot_checks(s, k, nprobe, metric, rq)) return rc;
    if (int rc = table_max_candidates(s, max_candidates)) return rc;
    if (d_tie_flags && k > 1023) return fail(PQV_ERR_UNSUPPORTED, "tie flags need a runner-up entry: k <= 1023");
    if (rq && rq->groups.size && grouped_beyond_kernel_lists(s, k, rq->groups.size, nprobe))
        return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_grouped_device takes k * group_size <= 1024 and at most 1024 probed lists per query");
    if (beyond_kernel_lists(s, k, nprobe))
        return fail(PQV_ERR_UNSUPPORTED, s->n_files ? "the device entry points take k <= 1024 and at most 1024 probed lists per query (the sum of "
                                                      "min(nprobe, n_clusters) over the table's files; pqv_topk has no such limit)"
                                                    : "the device entry points take k <= 1024 and min(nprobe, n_clusters) <= 1024 (pqv_topk has no such limit)");
    if (nq == 0) return PQV_OK;
    if (!d_queries || !d_row_idx || !d_dist) return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
    if (int rc = use_device(s->device)) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    Lane lane;
    if (metric == PQV_COSINE) {
        // n(q), then the L2 call of the cosine searcher on the same stream
        if (int rc = cosine_queries_device(s, static_cast<const float *>(d_queries), nq, stream, lane)) return rc;
        if (int rc = pqv_topk_device_impl(s->cos.get(), lane->s_qcos.p, nq, k, nprobe, max_candidates, PQV_L2SQ_REF4, 2, d_row_idx, d_dist,
                                          d_n_found, d_n_candidates, d_tie_flags, stream, rq))
            return rc;
        return lane.release();
    }
    if (int rc = lane.acquire(s, stream)) return rc;
    // with flags the kernels carry one extra merged entry (the runner-up), exactly as pqv_topk does
    // (PQV_DOT: no runner-up -- dot_merge_kernel writes the flags with zeros)
    if (int rc = enqueue_topk(s, static_cast<const float *>(d_queries), nq, (d_tie_flags && metric != PQV_DOT) ? k + 1 : k, k, nprobe, max_candidates,
                              metric, sqrt_out, static_cast<uint32_t *>(d_row_idx),
                              static_cast<float *>(d_dist), static_cast<uint32_t *>(d_n_found),
                              static_cast<uint64_t *>(d_n_candidates), static_cast<uint32_t *>(d_tie_flags), stream, *lane, rq))
        return rc;
    s->counters.queries += nq;
    return lane.release();
}
extern "C" int pqv_topk_device(const pqv_searcher *s, const void *d_queries, uint32_t nq, uint32_t k,
                               uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                               void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                               void *hip_stream) {
    return guard([&] { return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found, d_n_candidates, nullptr, hip_stream); });
}
extern "C" int pqv_topk_device_flags(const pqv_searcher *s, const void *d_queries, uint32_t nq, uint32_t k,
                                     uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                     void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                                     void *d_tie_flags, void *hip_stream) {
    if (!d_tie_flags) return fail(PQV_ERR_INVALID, "d_tie_flags must not be NULL");
    return guard([&] { return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found, d_n_candidates, d_tie_flags, hip_stream); });
}

// ---- host sub-batches ------------------------------------------------------------------------------------------------
// One per-query output of a host top-k call: `bytes` per query, written by a sub-batch's kernels to `buf` and copied from there to
// the caller's array at the sub-batch's offset (dst NULL: the buffer is sized, nothing is copied).
struct BatchOut { DevBuf *buf; size_t bytes; void *dst; };
// The loop of every host top-k entry point: the queries go through the lane in sub-batches of at most `batch` (the caller's bound
// on its scratch).  Per sub-batch [q0, q0 + b): the queries uploaded to s_queries (through the pinned `h_stage` where the caller
// has one), the slice of a per-query filter uploaded and the sub-batch's copy of the request pointed at it (upload_query_filter:
// IN lims rebased), enqueue(b, brq) -- brq: that copy, for the caller to add its device outputs to, or nullptr for a call without a
// request --, every output copied back, ONE synchronise, after(q0, b) on the host, and the queries counted.  s_queries and the
// outputs' buffers are sized here, for `batch`, before the first enqueue.
template <class Enqueue, class After>
static int host_batches(const pqv_searcher *s, Scratch &sc, const float *queries, uint32_t nq, uint32_t batch, const SearchRequest *rq,
                        void *h_stage, const std::vector<BatchOut> &outs, Enqueue enqueue, After after) {
    const size_t q_row = static_cast<size_t>(s->dim) * sizeof(float);
    HIP_TRY(sc.s_queries.ensure(batch * q_row));
    for (const BatchOut &o : outs) HIP_TRY(o.buf->ensure(batch * o.bytes));
    SearchRequest sub{};
    if (rq) sub = *rq;
    std::vector<uint64_t> sub_lims;      // (an IN filter's rebased lims stay alive until the sub-batch's synchronisation)
    for (uint32_t q0 = 0; q0 < nq; q0 += batch) {
        const uint32_t b = std::min<uint32_t>(batch, nq - q0);
        if (int rc = upload_query_filter(sc, rq, sub, q0, b, sub_lims, s->stream)) return rc;
        if (rq && rq->expand.h_depths) {       // (pqv_topk_depth: the sub-batch's given depths)
            HIP_TRY(sc.s_depths.ensure(static_cast<size_t>(b) * sizeof(uint32_t)));
            HIP_TRY(hipMemcpyAsync(sc.s_depths.p, rq->expand.h_depths + q0, static_cast<size_t>(b) * sizeof(uint32_t), hipMemcpyHostToDevice, s->stream));
            sub.expand.d_depths = sc.s_depths.as<uint32_t>();
        }
        const void *src = queries + static_cast<uint64_t>(q0) * s->dim;
        if (h_stage) src = std::memcpy(h_stage, src, b * q_row);
        HIP_TRY(hipMemcpyAsync(sc.s_queries.p, src, b * q_row, hipMemcpyHostToDevice, s->stream));
        if (int rc = enqueue(b, rq ? &sub : nullptr)) return rc;
        for (const BatchOut &o : outs)
            if (o.dst) HIP_TRY(hipMemcpyAsync(static_cast<char *>(o.dst) + q0 * o.bytes, o.buf->p, b * o.bytes, hipMemcpyDeviceToHost, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        if (int rc = after(q0, b)) return rc;
        s->counters.queries += b;
    }
    return PQV_OK;
}

namespace {
int distinct_unbounded(const pqv_searcher *s, Scratch &sc, const SearchRequest *mv, const float *queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                       uint64_t max_candidates, int metric, int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key,
                       uint32_t *n_found, uint64_t *n_candidates, uint32_t m, uint32_t *group_rows);
}
// The body of every host top-k entry point.  A grouping (rq->distinct(): pqv_topk_distinct / pqv_topk_grouped and their filtered and
// expanding forms) changes what is read from the request below: rows per query k * m (row_idx / dist [nq, k, m]; m = groups.size,
// 1 for a distinct call), the group_key / group_rows outputs [nq, k], no runner-up entry and no tie replay, and distinct_unbounded
// beyond the kernels' lists.
static int pqv_topk_impl(const pqv_searcher *s, const float *queries, uint32_t nq, uint32_t query_len,
                        uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                        uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates, const SearchRequest *rq = nullptr,
                        int64_t *group_key = nullptr, uint32_t *group_rows = nullptr) {
    if (int rc = validate_query(s, k, nprobe, metric, max_candidates, query_len)) return rc;
    if (int rc = dot_checks(s, k, nprobe, metric, rq)) return rc;
    if (nq == 0) return PQV_OK;
    if (!queries || !row_idx || !dist) return fail(PQV_ERR_INVALID, "queries/row_idx/dist must not be NULL");
    if (int rc = use_device(s->device)) return rc;
    std::vector<float> nq_host;
    if (int rc = cosine_queries_host(s, queries, nq, metric, sqrt_out, nq_host)) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    // One extra merged entry (the runner-up) lets the merge kernel see ties at the k-th
    // distance; queries it flags are replayed through the exact heap (replay_query_exact).
    // (k == UINT32_MAX -- "keep everything": the reference takes any NonZeroUsize -- must not wrap to a plan with k = 0)
    // (PQV_DOT: no runner-up, no replay -- the order is (dist, position) and the flags come back zero; its limits were checked above)
    const bool dot = metric == PQV_DOT, grouped = rq && rq->distinct();
    const bool expand = rq && rq->expanding();      // (the expanding forms stay within the kernels' lists: checked by their views)
    const uint32_t m = grouped ? std::max<uint32_t>(1, rq->groups.size) : 1;
    const uint32_t k_int = (dot || grouped || k >= 1024u) ? k : k + 1;
    Lane lane;
    if (int rc = lane.acquire(s, s->stream)) return rc;
    Scratch &sc = *lane;
    if (grouped ? !expand && grouped_beyond_kernel_lists(s, k, m, nprobe) : !dot && (k >= 1024u || beyond_kernel_lists(s, k_int, nprobe))) {
        if (int rc = grouped ? distinct_unbounded(s, sc, rq, queries, nq, k, nprobe, max_candidates, metric, sqrt_out, row_idx, dist, group_key,
                                                  n_found, n_candidates, m, group_rows)
                             : topk_unbounded(s, sc, queries, nq, k, nprobe, max_candidates, metric, sqrt_out, row_idx, dist, n_found, n_candidates, rq))
            return rc;
        return lane.release();
    }
    // bound the scratch: sub-batch so the per-wave partial lists stay under ~1 GiB
    // (per query: partial lists, probe partial lists, candidate buffer, the int8 images of its probed pairs; a grouping: 20 B per
    //  entry of the partial lists, and a grouped call's second pass 16 B per entry of k * m in the same buffers)
    const TopkPlan p1 = plan_topk(s, std::min<uint32_t>(nq, 1024), probe_arg(rq, nprobe), k_int, metric, stream_request(rq));
    const uint64_t km = static_cast<uint64_t>(k) * m;
    const uint64_t per_query =
        grouped ? static_cast<uint64_t>(p1.n_part_rr) * std::max<uint64_t>(k * 20ull, m > 1 ? km * 16 + 4 : 0) +
                      static_cast<uint64_t>(p1.n_part_probe) * p1.probe_kpart * 12 +
                      static_cast<uint64_t>(p1.np) * 32 + static_cast<uint64_t>(s->sdim + s->dim) * 4 + 20ull * k + (m > 1 ? 8ull * km : 0) + 16
                : static_cast<uint64_t>(p1.n_part_rr) * k_int * 12 + static_cast<uint64_t>(p1.n_part_probe) * p1.probe_kpart * 12 +
                      static_cast<uint64_t>(cand_cap_for(s, k_int)) * 12 + static_cast<uint64_t>(p1.np) * (s->sdim + 32) +
                      static_cast<uint64_t>(s->sdim) * 4 + 1;
    const uint32_t batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(nq, (1ull << 30) / per_query)));
    // the tie replay reads the flags, n_found (which it corrects) and an expanding call's lists used: the caller's arrays, or the call's
    uint32_t *nf = n_found, *used = expand ? rq->expand.h_used : nullptr;
    std::vector<uint32_t> h_tie, h_nf, h_used;
    if (!grouped) {
        h_tie.resize(nq);
        if (!nf) { h_nf.resize(nq); nf = h_nf.data(); }
        if (expand && !used) { h_used.resize(nq); used = h_used.data(); }
    }
    // A plain call of a few queries (TopkBuilder::search is ONE) is six small pageable copies otherwise -- the query in, rows,
    // distances, counts and tie flags out, each staged and waited for by the runtime: 60-80 us around 180 us of kernels.  Small calls
    // go through ONE pinned buffer instead -- host memory the device can address: the queries are staged in it, and the kernels WRITE
    // the results straight into it as one block {candidates u64 | rows | dist | found | tie}, so there is no device-to-host copy
    // behind them, only the synchronise.
    const size_t q_bytes = static_cast<size_t>(batch) * s->dim * sizeof(float);
    const size_t out_bytes = static_cast<size_t>(batch) * (16 + 8 * static_cast<size_t>(k));
    // (the result block starts with the u64 candidate counts: its offset behind the queries is rounded up to 64 bytes -- batch * dim
    //  may be odd, and the kernels store 64-bit values there)
    const size_t out_off = (q_bytes + 63) & ~static_cast<size_t>(63);
    const bool small_io = !grouped && out_off + out_bytes <= (256u << 10);
    if (small_io) HIP_TRY(sc.h_io.ensure(out_off + out_bytes));
    std::vector<BatchOut> outs;
    if (!small_io)
        outs = {{&sc.s_rows, km * sizeof(uint32_t), row_idx}, {&sc.s_dist, km * sizeof(float), dist}, {&sc.s_nfound, sizeof(uint32_t), nf},
                {&sc.s_ncand, sizeof(uint64_t), n_candidates}};
    if (grouped) {
        outs.push_back({&sc.s_grp_out, k * sizeof(int64_t), group_key});
        if (group_rows) outs.push_back({&sc.s_grows_out, k * sizeof(uint32_t), group_rows});
    } else if (!small_io) {
        outs.push_back({&sc.s_tie, sizeof(uint32_t), h_tie.data()});
    }
    // (an expanding call: the lists each query used come back with its results)
    if (expand) outs.push_back({&sc.s_expand_used, sizeof(uint32_t), used});
    // the pinned block's arrays, laid out for a sub-batch of b queries
    struct Block { uint64_t *ncand; uint32_t *rows; float *dist; uint32_t *nf, *tie; };
    auto block = [&](uint32_t b) {
        char *ob = static_cast<char *>(sc.h_io.p) + out_off;
        uint32_t *f = reinterpret_cast<uint32_t *>(ob + 8ull * b + 8ull * b * k);
        return Block{reinterpret_cast<uint64_t *>(ob), reinterpret_cast<uint32_t *>(ob + 8ull * b), reinterpret_cast<float *>(ob + 8ull * b + 4ull * b * k),
                     f, f + b};
    };
    const uint32_t np = probe_count(s, probe_arg(rq, nprobe));
    if (int rc = host_batches(
            s, sc, queries, nq, batch, rq, small_io ? sc.h_io.p : nullptr, outs,
            [&](uint32_t b, SearchRequest *brq) {
                if (expand) brq->expand.d_used = sc.s_expand_used.as<uint32_t>();
                if (grouped) {
                    brq->groups.d_keys = sc.s_grp_out.as<int64_t>();
                    brq->groups.d_rows = group_rows ? sc.s_grows_out.as<uint32_t>() : nullptr;
                }
                const Block o = small_io ? block(b)
                                         : Block{sc.s_ncand.as<uint64_t>(), sc.s_rows.as<uint32_t>(), sc.s_dist.as<float>(), sc.s_nfound.as<uint32_t>(),
                                                 grouped ? nullptr : sc.s_tie.as<uint32_t>()};
                return enqueue_topk(s, sc.s_queries.as<float>(), b, k_int, k, nprobe, max_candidates, metric, sqrt_out, o.rows, o.dist, o.nf, o.ncand,
                                    o.tie, s->stream, sc, brq);
            },
            [&](uint32_t q0, uint32_t b) -> int {
                if (grouped) return PQV_OK;
                if (small_io) {
                    const Block o = block(b);
                    if (n_candidates) std::memcpy(n_candidates + q0, o.ncand, static_cast<size_t>(b) * sizeof(uint64_t));
                    std::memcpy(row_idx + static_cast<uint64_t>(q0) * k, o.rows, static_cast<size_t>(b) * k * sizeof(uint32_t));
                    std::memcpy(dist + static_cast<uint64_t>(q0) * k, o.dist, static_cast<size_t>(b) * k * sizeof(float));
                    std::memcpy(nf + q0, o.nf, static_cast<size_t>(b) * sizeof(uint32_t));
                    std::memcpy(h_tie.data() + q0, o.tie, static_cast<size_t>(b) * sizeof(uint32_t));
                }
                for (uint32_t i = 0; i < b; ++i) {      // (candidate_rows / embeddings_fetched are counted on the device)
                    const uint64_t q = static_cast<uint64_t>(q0) + i;
                    if (!h_tie[q]) continue;
                    // tied output distances: survivors / order follow Rust's heap mechanics exactly
                    RowFilter allow;
                    if (int rc = row_filter(s, rq, q, allow)) return rc;
                    if (int rc = replay_query_exact(s, sc, s->sdim != s->dim ? sc.s_qpad.as<float>() + static_cast<size_t>(i) * s->sdim
                                                                              : sc.s_queries.as<float>() + static_cast<size_t>(i) * s->dim, i,
                                                    expand ? std::min<uint32_t>(std::max<uint32_t>(1, used[q]), np) : np,
                                                    k, max_candidates, metric, sqrt_out, row_idx + q * k, dist + q * k, &nf[q], nprobe,
                                                    allow.active() ? &allow : nullptr, np))
                        return rc;
                    s->counters.exact_replays++;
                }
                return PQV_OK;
            }))
        return rc;
    return lane.release();
}
extern "C" int pqv_topk(const pqv_searcher *s, const float *queries, uint32_t nq, uint32_t query_len,
                        uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                        uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] { return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates); });
}

// ---- range search ----------------------------------------------------------------------------------------------------
// Every candidate within `radius` of each query (pqv.h: pqv_range_search).  Per sub-batch of queries: the probe (enqueue_probe;
// beyond the kernels' 1024-entry lists host_probe), ONE stream_kernel STREAM_RANGE pass that appends every hit
// to its query's segment, ONE synchronisation for the hit counts (the output is sized from them), then the segments sorted
// by (d2, candidate position) and written out on the device (kernels_range.hip) and copied back.
namespace {
struct HostFree { void operator()(void *p) const { std::free(p); } };

template <class T>
int grow_host(std::unique_ptr<T, HostFree> &buf, uint64_t &cap, uint64_t need) {
    if (need <= cap) return PQV_OK;
    const uint64_t n = std::max<uint64_t>(need, cap + cap / 2);
    void *p = std::realloc(buf.get(), static_cast<size_t>(n) * sizeof(T));
    if (!p) return fail(PQV_ERR_OOM, "host allocation failed");
    (void)buf.release();
    buf.reset(static_cast<T *>(p));
    cap = n;
    return PQV_OK;
}

// What follows a hit pass's synchronisation, for the b queries from q0 whose hit counts h_cnt came back: the output offsets from
// the counts (lims[q0 + 1 ..] from lims[q0]; n_within), the library buffers grown, the segments sorted by (distance key, position)
// and written out on the device -- one block each up to RANGE_SMALL hits, the multi-pass path beyond --, PQV_DOT's ord halves
// turned back into distances, and the results copied behind lims[q0] and waited for.  Segments: uniform (q * stride) or packed
// (d_seg_off, with the host's per-query room).  e_end: the timing event recorded behind the write-out, or nullptr.
struct RangeWriteOut {
    const uint32_t *d_hit_cnt;    // [b] on the device
    const uint32_t *h_cnt;        // [b] the same counts on the host
    const uint64_t *h_room;       // [b] entries each segment holds, or nullptr: `stride` each
    uint64_t stride;
    const uint64_t *d_seg_off;    // [b] on the device, or nullptr (RangeSortArgs::seg_off)
    uint64_t max_results;
    int metric, sqrt_out;
};
int range_write_out(const pqv_searcher *s, Scratch &sc, const RangeWriteOut &w, uint32_t q0, uint32_t b, uint64_t *lims,
                    std::unique_ptr<uint32_t, HostFree> &rows, std::unique_ptr<float, HostFree> &dist, uint64_t &cap_rows, uint64_t &cap_dist,
                    uint64_t *n_within, std::vector<uint64_t> &h_off, std::vector<pqv::RangeSeg> &segs, hipEvent_t e_end, uint32_t &launches) {
    using namespace pqv;
    hipStream_t st = s->stream;
    // output offsets from the counts; segments longer than one block's sort go to the multi-pass path
    segs.clear();
    uint64_t tot = 0, alt = 0;
    uint32_t max_n = 0;
    bool any_small = false;
    for (uint32_t i = 0; i < b; ++i) {
        const uint32_t n = w.h_cnt[i];
        if (n > (w.h_room ? w.h_room[i] : w.stride)) return fail(PQV_ERR_HIP, "range search: a segment overflowed");     // (cannot happen: n <= capped candidates)
        const uint64_t kept = w.max_results ? std::min<uint64_t>(n, w.max_results) : n;
        h_off[i] = tot;
        tot += kept;
        lims[q0 + i + 1] = lims[q0 + i] + kept;
        if (n_within) n_within[q0 + i] = n;
        if (n > RANGE_SMALL) { segs.push_back(RangeSeg{i, n, alt}); alt += n; max_n = std::max(max_n, n); }
        else if (n) any_small = true;
    }
    if (int rc = grow_host(rows, cap_rows, lims[q0 + b])) return rc;
    if (int rc = grow_host(dist, cap_dist, lims[q0 + b])) return rc;
    if (tot) {
        HIP_TRY(sc.s_rout_rows.ensure(tot * sizeof(uint32_t)));
        HIP_TRY(sc.s_rout_dist.ensure(tot * sizeof(float)));
        HIP_TRY(hipMemcpyAsync(sc.s_rout_off.p, h_off.data(), static_cast<size_t>(b) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
        RangeSortArgs sa{};
        sa.nq = b; sa.hit_cnt = w.d_hit_cnt;
        sa.keys = sc.s_hit_keys.as<uint64_t>(); sa.vals = sc.s_hit_vals.as<uint32_t>(); sa.seg_stride = w.stride; sa.seg_off = w.d_seg_off;
        sa.max_results = w.max_results; sa.out_off = sc.s_rout_off.as<uint64_t>();
        sa.ids = s->d_final_ids; sa.sqrt_out = w.sqrt_out;
        sa.out_rows = sc.s_rout_rows.as<uint32_t>(); sa.out_dist = sc.s_rout_dist.as<float>();
        if (any_small) { HIP_TRY(launch_range_sort_small(sa, st)); ++launches; }
        if (!segs.empty()) {
            HIP_TRY(sc.s_alt_keys.ensure(alt * sizeof(uint64_t)));
            HIP_TRY(sc.s_alt_vals.ensure(alt * sizeof(uint32_t)));
            HIP_TRY(sc.s_rsegs.ensure(segs.size() * sizeof(RangeSeg)));
            HIP_TRY(hipMemcpyAsync(sc.s_rsegs.p, segs.data(), segs.size() * sizeof(RangeSeg), hipMemcpyHostToDevice, st));
            sa.alt_keys = sc.s_alt_keys.as<uint64_t>(); sa.alt_vals = sc.s_alt_vals.as<uint32_t>();
            sa.segs = sc.s_rsegs.as<RangeSeg>(); sa.n_segs = static_cast<uint32_t>(segs.size());
            uint32_t nl = 0;
            HIP_TRY(launch_range_sort_large(sa, max_n, &nl, st));
            launches += nl;
        }
        if (w.metric == PQV_DOT) {     // (the sort kernels wrote the keys' ord halves: back to dist in place)
            HIP_TRY(launch_dot_finish(sc.s_rout_dist.as<float>(), tot, st));
            ++launches;
        }
        if (e_end) HIP_TRY(hipEventRecord(e_end, st));
        HIP_TRY(hipMemcpyAsync(rows.get() + lims[q0], sc.s_rout_rows.p, tot * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(dist.get() + lims[q0], sc.s_rout_dist.p, tot * sizeof(float), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
    } else if (e_end) {
        HIP_TRY(hipEventRecord(e_end, st));
    }
    return PQV_OK;
}

int range_body(const pqv_searcher *s, Scratch &sc, const float *queries, uint32_t nq, float radius, uint32_t nprobe,
               uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out, uint64_t *lims,
               std::unique_ptr<uint32_t, HostFree> &rows, std::unique_ptr<float, HostFree> &dist, uint64_t *n_within,
               uint64_t *n_candidates, const SearchRequest *rq = nullptr) {
    using namespace pqv;
    hipStream_t st = s->stream;
    const uint32_t kc = s->n_clusters, np = probe_count(s, nprobe);
    const bool wide_probe = np > 1024;              // (merge_kernel's lists hold up to 1024 probed clusters)
    // a query's segment holds its capped candidates: at most the np longest lists, at most max_candidates
    uint64_t bound = 0;
    {
        std::vector<uint64_t> len(kc);
        for (uint32_t c = 0; c < kc; ++c) len[c] = s->h_list_off[c + 1] - s->h_list_off[c];
        std::sort(len.begin(), len.end(), std::greater<uint64_t>());
        for (uint32_t j = 0; j < np; ++j) bound += len[j];
        if (max_candidates) bound = std::min(bound, max_candidates);
    }
    const uint64_t stride = std::max<uint64_t>(1, bound);
    // sub-batches: the segments (12 B per entry) and the probe's scratch within ~1 GiB, at most 65535 queries (gridDim.z);
    // a query whose segment alone is larger still runs, alone
    const TopkPlan p1 = plan_topk(s, std::min<uint32_t>(nq, 1024), nprobe, 1, metric);
    const uint64_t per_query = stride * 12 + static_cast<uint64_t>(p1.n_part_probe) * std::max<uint32_t>(64, np) * 12 +
                               static_cast<uint64_t>(np) * 12 + static_cast<uint64_t>(s->dim + s->sdim) * 4 + 32;
    const uint32_t batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>({nq, 65535ull, (1ull << 30) / per_query})));
    HIP_TRY(sc.s_queries.ensure(static_cast<size_t>(batch) * s->dim * sizeof(float)));
    if (s->sdim != s->dim) HIP_TRY(sc.s_qpad.ensure(static_cast<size_t>(batch) * s->sdim * sizeof(float)));
    HIP_TRY(sc.s_ncand.ensure(static_cast<size_t>(batch) * sizeof(uint64_t)));
    HIP_TRY(sc.s_hit_cnt.ensure(static_cast<size_t>(batch) * sizeof(uint32_t)));
    HIP_TRY(sc.s_hit_keys.ensure(static_cast<size_t>(batch) * stride * sizeof(uint64_t)));
    HIP_TRY(sc.s_hit_vals.ensure(static_cast<size_t>(batch) * stride * sizeof(uint32_t)));
    HIP_TRY(sc.s_rout_off.ensure(static_cast<size_t>(batch) * sizeof(uint64_t)));
    SearchRequest sub{};      // (a keyed call: each sub-batch's kernels read its own slice of the query keys)
    if (rq) sub = *rq;
    std::vector<uint64_t> sub_lims;
    std::vector<uint32_t> h_cnt(batch), h_probe;
    std::vector<uint64_t> h_ncand(batch), h_off(batch);
    std::vector<RangeSeg> segs;
    uint64_t cap_rows = 1, cap_dist = 1;      // entries the library buffers have room for
    const uint64_t max_len = std::max<uint64_t>(1, s->max_list_len);
    for (uint32_t q0 = 0; q0 < nq; q0 += batch) {
        const uint32_t b = std::min<uint32_t>(batch, nq - q0);
        uint32_t launches = 0;
        hipEvent_t e[4];     // pqv_timing_read: the STREAM_RANGE pass as the "re-rank", probe .. write-out as the total
        if (int rc = timing_events(s, e)) return rc;
        HIP_TRY(hipMemcpyAsync(sc.s_queries.p, queries + static_cast<uint64_t>(q0) * s->dim, static_cast<size_t>(b) * s->dim * sizeof(float),
                               hipMemcpyHostToDevice, st));
        if (int rc = upload_query_filter(sc, rq, sub, q0, b, sub_lims, st)) return rc;
        if (e[0]) HIP_TRY(hipEventRecord(e[0], st));
        const float *d_q = sc.s_queries.as<float>(), *d_q_s = d_q;
        if (s->sdim != s->dim) {
            HIP_TRY(launch_pad_rows(d_q, nullptr, b, s->dim, s->sdim, sc.s_qpad.as<float>(), st));
            d_q_s = sc.s_qpad.as<float>();
            ++launches;
        }
        if (!wide_probe) {
            const TopkPlan p = plan_topk(s, b, nprobe, 1, metric);
            MergeArgs pm{};
            if (int rc = probe_merge_args(s, sc, p, b, max_candidates, pm)) return rc;
            pm.stats = rq ? nullptr : s->d_stats.as<unsigned long long>();      // candidate_rows / embeddings_fetched, as a top-k call counts them
            if (int rc = enqueue_probe(s, sc, p, d_q, b, nprobe, max_candidates, pm, nullptr, 0, st, metric)) return rc;
            launches += 2;
        } else {
            // find_closest_centroids without the kernels' list limit (as topk_unbounded)
            if (int rc = host_probe(s, sc, d_q, b, nprobe, max_candidates, true, h_probe, h_ncand.data())) return rc;
            for (uint32_t i = 0; i < b; ++i) {
                s->counters.candidate_rows += h_ncand[i];                         // index_exec.rs:289-299
                if (!rq) s->counters.embeddings_fetched += max_candidates ? std::min<uint64_t>(h_ncand[i], max_candidates) : h_ncand[i];
            }
        }

        // the hits: one pass over every (query, probed list), rows through d_mat / d_row_of (every layout)
        HIP_TRY(hipMemsetAsync(sc.s_hit_cnt.p, 0, static_cast<size_t>(b) * sizeof(uint32_t), st));
        StreamArgs ra = stream_args(s, sc, d_q_s, b, np, 1, max_candidates, metric);
        stream_split(max_len, std::max<uint64_t>(1, static_cast<uint64_t>(b) * np), ra.rows_per_block, ra.blocks_per_list);   // (as the top-k form)
        ra.radius = radius; ra.sqrt_out = sqrt_out;
        ra.hit_cnt = sc.s_hit_cnt.as<uint32_t>(); ra.hit_keys = sc.s_hit_keys.as<uint64_t>(); ra.hit_vals = sc.s_hit_vals.as<uint32_t>();
        ra.seg_stride = stride;
        if (e[1]) HIP_TRY(hipEventRecord(e[1], st));
        for (uint32_t j0 = 0; j0 < np; j0 += 32768) {                    // gridDim.y <= 65535
            ra.j0 = j0; ra.nj = std::min<uint32_t>(32768, np - j0);
            // (a request: the considered rows are counted by the kernel; candidate_rows too unless the host probe counted it above)
            HIP_TRY(launch_stream_pass(ra, rq ? &sub : nullptr, s->d_stats.as<unsigned long long>(), wide_probe ? nullptr : sc.s_ncand.as<uint64_t>(),
                                       STREAM_RANGE, st));
            ++launches;
        }
        if (e[2]) HIP_TRY(hipEventRecord(e[2], st));
        HIP_TRY(hipMemcpyAsync(h_cnt.data(), sc.s_hit_cnt.p, static_cast<size_t>(b) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        if (!wide_probe)
            HIP_TRY(hipMemcpyAsync(h_ncand.data(), sc.s_ncand.p, static_cast<size_t>(b) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));

        if (n_candidates) std::copy(h_ncand.begin(), h_ncand.begin() + b, n_candidates + q0);
        RangeWriteOut wo{sc.s_hit_cnt.as<uint32_t>(), h_cnt.data(), nullptr, stride, nullptr, max_results, metric, sqrt_out};
        if (int rc = range_write_out(s, sc, wo, q0, b, lims, rows, dist, cap_rows, cap_dist, n_within, h_off, segs, e[3], launches)) return rc;
        s->counters.queries += b;
        s->counters.kernel_launches += launches;
    }
    return PQV_OK;
}
}  // namespace

static int pqv_range_search_impl(const pqv_searcher *s, const float *queries, uint32_t nq, uint32_t query_len, float radius,
                                 uint32_t nprobe, uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out,
                                 uint64_t **lims_out, uint32_t **rows_out, float **dist_out, uint64_t *n_within,
                                 uint64_t *n_candidates, const SearchRequest *rq = nullptr) {
    if (int rc = validate_query(s, 1, nprobe, metric, max_candidates, query_len)) return rc;
    if (int rc = dot_checks(s, 1, nprobe, metric, rq)) return rc;
    if (metric == PQV_DOT) sqrt_out = 0;      // (ignored: the range_* kernels run as order-only machinery)
    if (std::isnan(radius)) return fail(PQV_ERR_INVALID, "radius must not be NaN");
    if (!lims_out || !rows_out || !dist_out) return fail(PQV_ERR_INVALID, "lims/row_idx/dist must not be NULL");
    if (nq && !queries) return fail(PQV_ERR_INVALID, "queries must not be NULL");
    *lims_out = nullptr; *rows_out = nullptr; *dist_out = nullptr;
    std::unique_ptr<uint64_t, HostFree> lims(static_cast<uint64_t *>(std::malloc((static_cast<size_t>(nq) + 1) * sizeof(uint64_t))));
    std::unique_ptr<uint32_t, HostFree> rows(static_cast<uint32_t *>(std::malloc(sizeof(uint32_t))));
    std::unique_ptr<float, HostFree> dist(static_cast<float *>(std::malloc(sizeof(float))));
    if (!lims || !rows || !dist) return fail(PQV_ERR_OOM, "host allocation failed");
    lims.get()[0] = 0;
    std::vector<float> nq_host;
    if (nq) {
        if (int rc = use_device(s->device)) return rc;
        // (PQV_COSINE: the cosine searcher's range search over n(q): hits 0.5 d2 <= radius, written out halved)
        if (int rc = cosine_queries_host(s, queries, nq, metric, sqrt_out, nq_host)) return rc;
        std::lock_guard<std::mutex> lock(s->mu);
        Lane lane;
        if (int rc = lane.acquire(s, s->stream)) return rc;
        if (int rc = range_body(s, *lane, queries, nq, radius, nprobe, max_candidates, max_results, metric, sqrt_out, lims.get(), rows,
                                dist, n_within, n_candidates, rq))
            return rc;
        if (int rc = lane.release()) return rc;
    }
    *lims_out = lims.release(); *rows_out = rows.release(); *dist_out = dist.release();
    return PQV_OK;
}
extern "C" int pqv_range_search(const pqv_searcher *s, const float *queries, uint32_t nq, uint32_t query_len, float radius,
                                uint32_t nprobe, uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out,
                                uint64_t **lims, uint32_t **row_idx, float **dist, uint64_t *n_within, uint64_t *n_candidates) {
    return guard([&] { return pqv_range_search_impl(s, queries, nq, query_len, radius, nprobe, max_candidates, max_results, metric,
                                                    sqrt_out ? 1 : 0, lims, row_idx, dist, n_within, n_candidates); });
}
extern "C" void pqv_range_free(uint64_t *lims, uint32_t *row_idx, float *dist) {
    std::free(lims); std::free(row_idx); std::free(dist);
}

// ---- row masks (pqv.h: pqv_row_mask) -----------------------------------------------------------------------------------
// Creation: the allow bytes (host: through a temporary device copy; device: as given) -> mask_layout_kernel -> the position image
// and the allowed total, mask_pack_kernel -> the row image, and the row-order bytes kept on the host for the replays.  Complete
// on return.
static int row_mask_create_impl(const pqv_searcher *s, const uint8_t *h_allowed, const void *d_allowed, uint64_t n_rows, void *hip_stream,
                                pqv_row_mask **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    const uint64_t corpus_rows = s->corpus ? s->corpus->n : 0;
    if (n_rows != corpus_rows)
        return fail(PQV_ERR_INVALID, "row mask has " + std::to_string(n_rows) + " rows, the corpus has " + std::to_string(corpus_rows));
    if (n_rows && !h_allowed && !d_allowed) return fail(PQV_ERR_INVALID, "allowed must not be NULL");
    if (int rc = use_device(s->device)) return rc;
    std::unique_ptr<pqv_row_mask> m(new (std::nothrow) pqv_row_mask());
    if (!m) return fail(PQV_ERR_OOM, "host allocation failed");
    m->owner = s; m->owner_uid = s->uid; m->device = s->device; m->n_rows = n_rows;
    m->host.resize(n_rows);
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    const uint64_t n_words = (s->n + 63) / 64 + 1;
    const uint64_t row_words = (n_rows + 63) / 64;
    HIP_TRY(m->d_bits.alloc((n_words + 1) * sizeof(uint64_t)));
    HIP_TRY(m->d_rowbits.alloc(row_words * sizeof(uint64_t)));
    unsigned long long *d_count = m->d_bits.as<unsigned long long>() + n_words;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    DevBuf d_tmp;
    const uint8_t *d_src = static_cast<const uint8_t *>(d_allowed);
    if (h_allowed) {
        if (n_rows) std::memcpy(m->host.data(), h_allowed, n_rows);
        HIP_TRY(d_tmp.alloc(n_rows));
        if (n_rows) HIP_TRY(hipMemcpyAsync(d_tmp.p, h_allowed, n_rows, hipMemcpyHostToDevice, stream));
        d_src = d_tmp.as<uint8_t>();
    } else if (n_rows) {
        HIP_TRY(hipMemcpyAsync(m->host.data(), d_allowed, n_rows, hipMemcpyDeviceToHost, stream));
    }
    HIP_TRY(pqv::launch_mask_layout(d_src, n_rows, s->d_ids.as<uint32_t>(), s->n, m->d_bits.as<uint64_t>(), n_words, d_count, stream));
    HIP_TRY(pqv::launch_mask_pack(d_src, n_rows, m->d_rowbits.as<uint64_t>(), row_words, stream));
    unsigned long long h_count = 0;
    HIP_TRY(hipMemcpyAsync(&h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));       // (d_tmp is released at scope exit)
    m->count = h_count;
    m->host_ready.store(true, std::memory_order_release);
    *out = m.release();
    return PQV_OK;
}
extern "C" int pqv_row_mask_create(const pqv_searcher *s, const uint8_t *allowed, uint64_t n_rows, pqv_row_mask **out) {
    return guard([&] {
        if (out) *out = nullptr;
        if (s && out && n_rows && !allowed) return fail(PQV_ERR_INVALID, "allowed must not be NULL");
        static const uint8_t none = 0;
        return row_mask_create_impl(s, allowed ? allowed : &none, nullptr, n_rows, nullptr, out);
    });
}
extern "C" int pqv_row_mask_from_device(const pqv_searcher *s, const void *d_allowed, uint64_t n_rows, void *hip_stream, pqv_row_mask **out) {
    return guard([&] { return row_mask_create_impl(s, nullptr, d_allowed, n_rows, hip_stream, out); });
}
extern "C" uint64_t pqv_row_mask_rows(const pqv_row_mask *m) { return m ? m->n_rows : 0; }
extern "C" uint64_t pqv_row_mask_count(const pqv_row_mask *m) { return m ? m->count : 0; }
extern "C" void pqv_row_mask_free(pqv_row_mask *m) {
    if (!m) return;
    (void)hipSetDevice(m->device);
    delete m;
}
static int pqv_row_mask_to_bytes_impl(const pqv_row_mask *m, uint8_t *allowed, uint64_t n_rows) {
    if (!m) return fail(PQV_ERR_INVALID, "row mask must not be NULL");
    if (n_rows != m->n_rows)
        return fail(PQV_ERR_INVALID, "row mask has " + std::to_string(m->n_rows) + " rows, the buffer has " + std::to_string(n_rows));
    if (n_rows && !allowed) return fail(PQV_ERR_INVALID, "allowed must not be NULL");
    return row_image_to_bytes(m, allowed);       // (the row image of every mask, byte-made ones included; never the cached bytes)
}
extern "C" int pqv_row_mask_to_bytes(const pqv_row_mask *m, uint8_t *allowed, uint64_t n_rows) {
    return guard([&] { return pqv_row_mask_to_bytes_impl(m, allowed, n_rows); });
}

// ---- resident scalar columns and predicate masks (pqv.h: pqv_column, pqv_row_mask_from_predicates) ----------------------
struct pqv_column {
    int device = 0;
    int dtype = 0;
    uint64_t n = 0;
    void *d_values = nullptr;          // [n] of dtype
    uint8_t *d_valid = nullptr;        // optional [n] validity bytes (0 = NULL)
    bool owned = true;
    ~pqv_column() {
        if (owned) {
            if (d_values) (void)hipFree(d_values);
            if (d_valid) (void)hipFree(d_valid);
        }
    }
};
static size_t column_value_size(int dtype) { return (dtype == PQV_COL_I32 || dtype == PQV_COL_F32) ? 4 : 8; }

static int pqv_column_make(int device, int dtype, const void *values, const void *valid, uint64_t n_rows, bool upload, pqv_column **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (dtype != PQV_COL_I32 && dtype != PQV_COL_I64 && dtype != PQV_COL_F32 && dtype != PQV_COL_F64)
        return fail(PQV_ERR_INVALID, "unknown column type");
    if (n_rows > 0xFFFFFFFFull) return fail(PQV_ERR_UNSUPPORTED, "row ids are u32: at most 4294967295 rows per corpus");
    if (n_rows && !values) return fail(PQV_ERR_INVALID, upload ? "values must not be NULL" : "d_values must not be NULL");
    if (int rc = use_device(device)) return rc;
    std::unique_ptr<pqv_column> c(new (std::nothrow) pqv_column());
    if (!c) return fail(PQV_ERR_OOM, "host allocation failed");
    c->device = device; c->dtype = dtype; c->n = n_rows;
    if (!upload) {
        c->owned = false;
        c->d_values = const_cast<void *>(values);
        c->d_valid = static_cast<uint8_t *>(const_cast<void *>(valid));
    } else {
        const size_t vb = static_cast<size_t>(n_rows) * column_value_size(dtype);
        HIP_TRY(hipMalloc(&c->d_values, vb ? vb : 16));
        if (vb) HIP_TRY(hipMemcpy(c->d_values, values, vb, hipMemcpyHostToDevice));
        if (valid) {
            void *dv = nullptr;
            HIP_TRY(hipMalloc(&dv, n_rows ? n_rows : 16));
            c->d_valid = static_cast<uint8_t *>(dv);
            if (n_rows) HIP_TRY(hipMemcpy(c->d_valid, valid, n_rows, hipMemcpyHostToDevice));
        }
    }
    *out = c.release();
    return PQV_OK;
}
extern "C" int pqv_column_upload(int device, int dtype, const void *values, const uint8_t *valid, uint64_t n_rows, pqv_column **out) {
    return guard([&] { return pqv_column_make(device, dtype, values, valid, n_rows, true, out); });
}
extern "C" int pqv_column_from_device(int device, int dtype, const void *d_values, const void *d_valid, uint64_t n_rows, pqv_column **out) {
    return guard([&] { return pqv_column_make(device, dtype, d_values, d_valid, n_rows, false, out); });
}
extern "C" uint64_t pqv_column_rows(const pqv_column *c) { return c ? c->n : 0; }
extern "C" int pqv_column_dtype(const pqv_column *c) { return c ? c->dtype : -1; }
extern "C" int pqv_column_device(const pqv_column *c) { return c ? c->device : -1; }
extern "C" void pqv_column_free(pqv_column *c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    delete c;
}

// the postfix program of a predicate: 0..31 push leaf i, PQV_PRED_AND / PQV_PRED_OR fold the two top values
static int predicate_check(const uint8_t *program, uint32_t program_len, uint32_t n_leaves, uint32_t *max_depth) {
    if (max_depth) *max_depth = 0;
    if (program_len == 0) return fail(PQV_ERR_INVALID, "predicate program is empty");
    if (!program) return fail(PQV_ERR_INVALID, "program must not be NULL");
    if (n_leaves > 32) return fail(PQV_ERR_INVALID, "predicate has " + std::to_string(n_leaves) + " leaves, at most 32");
    uint32_t depth = 0, deepest = 0;
    bool ok = program_len <= 63;
    for (uint32_t i = 0; ok && i < program_len; ++i) {
        const uint8_t c = program[i];
        if (c == PQV_PRED_AND || c == PQV_PRED_OR) {
            if (depth < 2) ok = false; else --depth;
        } else if (c < 32 && c < n_leaves) {
            if (++depth > 32) ok = false;
            deepest = std::max(deepest, depth);
        } else {
            ok = false;
        }
    }
    if (!ok || depth != 1) return fail(PQV_ERR_INVALID, "predicate program is malformed");
    if (max_depth) *max_depth = deepest;
    return PQV_OK;
}
extern "C" int pqv_predicate_check(const uint8_t *program, uint32_t program_len, uint32_t n_leaves, uint32_t *max_depth) {
    return guard([&] { return predicate_check(program, program_len, n_leaves, max_depth); });
}

// (the kernels' leaf table takes ops and column types as the header numbers them)
static_assert(pqv::PRED_COL_I32 == PQV_COL_I32 && pqv::PRED_COL_I64 == PQV_COL_I64 && pqv::PRED_COL_F32 == PQV_COL_F32 &&
              pqv::PRED_COL_F64 == PQV_COL_F64, "kernels.h PRED_COL_* must equal pqv.h PQV_COL_*");
static_assert(pqv::PRED_EQ == PQV_OP_EQ && pqv::PRED_NE == PQV_OP_NE && pqv::PRED_LT == PQV_OP_LT && pqv::PRED_LE == PQV_OP_LE &&
              pqv::PRED_GT == PQV_OP_GT && pqv::PRED_GE == PQV_OP_GE && pqv::PRED_BETWEEN == PQV_OP_BETWEEN &&
              pqv::PRED_IS_NULL == PQV_OP_IS_NULL && pqv::PRED_MASK == PQV_OP_MASK && pqv::PRED_NOT == PQV_OP_NOT,
              "kernels.h PRED_* ops must equal pqv.h PQV_OP_*");
static_assert(pqv::PRED_PROG_AND == PQV_PRED_AND && pqv::PRED_PROG_OR == PQV_PRED_OR, "kernels.h PRED_PROG_* must equal pqv.h PQV_PRED_*");
static_assert(sizeof(pqv::PredArgs::program) == 64, "the program field holds 64 bytes");

// predicate_rows_kernel -> the row image, mask_gather_kernel -> the position image and the allowed total.  Host traffic: the
// kernel arguments in, the 8-byte total out; the row-order host bytes of the replays are made on first need (mask_host_bytes).
static int row_mask_from_predicates_impl(const pqv_searcher *s, uint32_t n_leaves, const pqv_column *const *columns,
                                         const pqv_row_mask *const *masks, const uint32_t *ops, const uint64_t *operands,
                                         const uint8_t *program, uint32_t program_len, void *hip_stream, pqv_row_mask **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (int rc = predicate_check(program, program_len, n_leaves, nullptr)) return rc;
    if (!ops) return fail(PQV_ERR_INVALID, "ops must not be NULL");
    if (!operands) return fail(PQV_ERR_INVALID, "operands must not be NULL");
    const uint64_t corpus_rows = s->corpus ? s->corpus->n : 0;
    pqv::PredArgs pa{};
    for (uint32_t i = 0; i < n_leaves; ++i) {
        const uint32_t op = ops[i] & ~static_cast<uint32_t>(PQV_OP_NOT);
        if (op > PQV_OP_MASK) return fail(PQV_ERR_INVALID, "unknown predicate op");
        pqv::PredLeaf &L = pa.leaf[i];
        L.op = ops[i]; L.a = operands[2 * i]; L.b = operands[2 * i + 1];
        if (op == PQV_OP_MASK) {
            const pqv_row_mask *lm = masks ? masks[i] : nullptr;
            if (!lm) return fail(PQV_ERR_INVALID, "row mask must not be NULL");
            if (lm->owner != s || lm->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "row mask belongs to another searcher");
            L.values = lm->d_rowbits.p; L.valid = nullptr; L.dtype = 0;
            continue;
        }
        const pqv_column *c = columns ? columns[i] : nullptr;
        if (!c) return fail(PQV_ERR_INVALID, "predicate leaf " + std::to_string(i) + " has no column");
        if (c->n != corpus_rows)
            return fail(PQV_ERR_INVALID, "column has " + std::to_string(c->n) + " rows, the corpus has " + std::to_string(corpus_rows));
        if (c->device != s->device)
            return fail(PQV_ERR_INVALID, "column is on device " + std::to_string(c->device) + ", the searcher on device " + std::to_string(s->device));
        L.values = c->d_values; L.valid = c->d_valid; L.dtype = static_cast<uint32_t>(c->dtype);
    }
    std::memcpy(pa.program, program, program_len);
    pa.program_len = program_len; pa.n_leaves = n_leaves; pa.n_rows = corpus_rows;
    if (int rc = use_device(s->device)) return rc;
    std::unique_ptr<pqv_row_mask> m(new (std::nothrow) pqv_row_mask());
    if (!m) return fail(PQV_ERR_OOM, "host allocation failed");
    m->owner = s; m->owner_uid = s->uid; m->device = s->device; m->n_rows = corpus_rows;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    const uint64_t n_words = (s->n + 63) / 64 + 1;
    const uint64_t row_words = (corpus_rows + 63) / 64;
    HIP_TRY(m->d_bits.alloc((n_words + 1) * sizeof(uint64_t)));
    HIP_TRY(m->d_rowbits.alloc(row_words * sizeof(uint64_t)));
    pa.rowbits = m->d_rowbits.as<uint64_t>(); pa.n_words = row_words;
    unsigned long long *d_count = m->d_bits.as<unsigned long long>() + n_words;
    HIP_TRY(hipMemsetAsync(d_count, 0, sizeof(unsigned long long), stream));
    if (row_words) HIP_TRY(pqv::launch_predicate_rows(pa, stream));
    HIP_TRY(pqv::launch_mask_gather(m->d_rowbits.as<uint64_t>(), corpus_rows, s->d_ids.as<uint32_t>(), s->n, m->d_bits.as<uint64_t>(), n_words,
                                    d_count, stream));
    unsigned long long h_count = 0;
    HIP_TRY(hipMemcpyAsync(&h_count, d_count, sizeof h_count, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    m->count = h_count;
    *out = m.release();
    return PQV_OK;
}
extern "C" int pqv_row_mask_from_predicates(const pqv_searcher *s, uint32_t n_leaves, const pqv_column *const *columns,
                                            const pqv_row_mask *const *masks, const uint32_t *ops, const uint64_t *operands,
                                            const uint8_t *program, uint32_t program_len, void *hip_stream, pqv_row_mask **out) {
    return guard([&] { return row_mask_from_predicates_impl(s, n_leaves, columns, masks, ops, operands, program, program_len, hip_stream, out); });
}

// the checks every masked entry point makes before anything else (after the searcher's own NULL check)
static int mask_view(const pqv_searcher *s, const pqv_row_mask *mask, SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!mask) return fail(PQV_ERR_INVALID, "row mask must not be NULL");
    if (mask->owner != s || mask->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "row mask belongs to another searcher");
    mv = SearchRequest{};
    mv.rows.bits = mask->d_bits.as<uint64_t>(); mv.rows.mask = mask;
    return PQV_OK;
}
extern "C" int pqv_topk_masked(const pqv_searcher *s, const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len,
                               uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                               uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = mask_view(s, mask, mv)) return rc;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates, &mv);
    });
}
extern "C" int pqv_topk_masked_device(const pqv_searcher *s, const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k,
                                      uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                      void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                                      void *d_tie_flags, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = mask_view(s, mask, mv)) return rc;
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, d_tie_flags, hip_stream, &mv);
    });
}
extern "C" int pqv_range_search_masked(const pqv_searcher *s, const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len,
                                       float radius, uint32_t nprobe, uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out,
                                       uint64_t **lims, uint32_t **row_idx, float **dist, uint64_t *n_within, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = mask_view(s, mask, mv)) return rc;
        return pqv_range_search_impl(s, queries, nq, query_len, radius, nprobe, max_candidates, max_results, metric, sqrt_out ? 1 : 0, lims,
                                     row_idx, dist, n_within, n_candidates, &mv);
    });
}

// ---- per-query key filters (pqv.h: pqv_row_keys) ------------------------------------------------------------------------
// Creation: ONE key_layout_kernel pass, a gather of the column through d_ids into the position image.  Complete on return.
static int row_keys_create_impl(const pqv_searcher *s, const pqv_column *c, void *hip_stream, pqv_row_keys **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!c) return fail(PQV_ERR_INVALID, "column must not be NULL");
    if (c->dtype != PQV_COL_I32 && c->dtype != PQV_COL_I64) return fail(PQV_ERR_INVALID, "key column must be PQV_COL_I32 or PQV_COL_I64");
    const uint64_t corpus_rows = s->corpus ? s->corpus->n : 0;
    if (c->n != corpus_rows)
        return fail(PQV_ERR_INVALID, "column has " + std::to_string(c->n) + " rows, the corpus has " + std::to_string(corpus_rows));
    if (c->device != s->device)
        return fail(PQV_ERR_INVALID, "column is on device " + std::to_string(c->device) + ", the searcher on device " + std::to_string(s->device));
    if (int rc = use_device(s->device)) return rc;
    std::unique_ptr<pqv_row_keys> kk(new (std::nothrow) pqv_row_keys());
    if (!kk) return fail(PQV_ERR_OOM, "host allocation failed");
    kk->owner = s; kk->owner_uid = s->uid; kk->device = s->device; kk->dtype = c->dtype;
    kk->n_rows = corpus_rows; kk->n_pos = s->n; kk->has_valid = c->d_valid != nullptr;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    const uint32_t es = static_cast<uint32_t>(column_value_size(c->dtype));
    const uint64_t n_words = (s->n + 63) / 64 + 1;
    HIP_TRY(kk->d_key_pos.alloc(n_words * 64 * es));
    if (kk->has_valid) HIP_TRY(kk->d_valid_pos.alloc(n_words * sizeof(uint64_t)));
    HIP_TRY(pqv::launch_key_layout(c->d_values, c->d_valid, es, corpus_rows, s->d_ids.as<uint32_t>(), s->n, kk->d_key_pos.p,
                                   kk->has_valid ? kk->d_valid_pos.as<uint64_t>() : nullptr, n_words, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    *out = kk.release();
    return PQV_OK;
}
extern "C" int pqv_row_keys_create(const pqv_searcher *s, const pqv_column *column, void *hip_stream, pqv_row_keys **out) {
    return guard([&] { return row_keys_create_impl(s, column, hip_stream, out); });
}
extern "C" uint64_t pqv_row_keys_rows(const pqv_row_keys *k) { return k ? k->n_rows : 0; }
extern "C" int pqv_row_keys_dtype(const pqv_row_keys *k) { return k ? k->dtype : -1; }
extern "C" void pqv_row_keys_free(pqv_row_keys *k) {
    if (!k) return;
    (void)hipSetDevice(k->device);
    delete k;
}

// the checks every keyed entry point makes before anything else: NULL handles first, nothing dereferenced before them
static int keyed_view(const pqv_searcher *s, const pqv_row_keys *keys, const void *qkeys, uint32_t nq, const pqv_row_mask *mask, SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!keys) return fail(PQV_ERR_INVALID, "row keys must not be NULL");
    if (nq && !qkeys) return fail(PQV_ERR_INVALID, "query keys must not be NULL");
    if (keys->owner != s || keys->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "row keys belong to another searcher");
    mv = SearchRequest{};
    if (mask) {
        if (int rc = mask_view(s, mask, mv)) return rc;
    }
    mv.rows.keys = keys;
    return PQV_OK;
}
extern "C" int pqv_topk_keyed(const pqv_searcher *s, const pqv_row_keys *keys, const int64_t *qkeys, const pqv_row_mask *mask,
                              const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates,
                              int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = keyed_view(s, keys, qkeys, nq, mask, mv)) return rc;
        mv.rows.h_qkeys = qkeys;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates, &mv);
    });
}
extern "C" int pqv_topk_keyed_device(const pqv_searcher *s, const pqv_row_keys *keys, const void *d_qkeys, const pqv_row_mask *mask,
                                     const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric,
                                     int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                                     void *d_tie_flags, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = keyed_view(s, keys, d_qkeys, nq, mask, mv)) return rc;
        mv.rows.d_qkeys = static_cast<const int64_t *>(d_qkeys);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, d_tie_flags, hip_stream, &mv);
    });
}
extern "C" int pqv_range_search_keyed(const pqv_searcher *s, const pqv_row_keys *keys, const int64_t *qkeys, const pqv_row_mask *mask,
                                      const float *queries, uint32_t nq, uint32_t query_len, float radius, uint32_t nprobe,
                                      uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out, uint64_t **lims,
                                      uint32_t **row_idx, float **dist, uint64_t *n_within, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = keyed_view(s, keys, qkeys, nq, mask, mv)) return rc;
        mv.rows.h_qkeys = qkeys;
        return pqv_range_search_impl(s, queries, nq, query_len, radius, nprobe, max_candidates, max_results, metric, sqrt_out ? 1 : 0, lims,
                                     row_idx, dist, n_within, n_candidates, &mv);
    });
}

// ---- per-query filters beyond equality (pqv.h: pqv_key_filter) ---------------------------------------------------------------
// The descriptor's checks, ahead of keyed_view's; `host`: a and b are host arrays and a set filter is validated in full.  On
// success the view carries the filter: PQV_KEY_EQ as the keyed calls' query keys, the other kinds in fkind / h_f* / d_f*.
static int filter_descriptor_checks(const pqv_key_filter *f, uint32_t nq, bool host) {
    if (!f) return fail(PQV_ERR_INVALID, "filter must not be NULL");
    if (f->kind > PQV_KEY_IN) return fail(PQV_ERR_INVALID, "unknown key filter kind " + std::to_string(f->kind));
    const bool reads_b = f->kind != PQV_KEY_EQ;
    if (nq && (!f->a || (reads_b && !f->b))) return fail(PQV_ERR_INVALID, "query keys must not be NULL");
    if (host && nq && f->kind == PQV_KEY_IN) {
        const uint64_t *lims = static_cast<const uint64_t *>(f->a);
        const int64_t *vals = static_cast<const int64_t *>(f->b);
        if (lims[0] != 0) return fail(PQV_ERR_INVALID, "query key sets must start at 0 and not decrease");
        for (uint32_t q = 0; q < nq; ++q)
            if (lims[q + 1] < lims[q]) return fail(PQV_ERR_INVALID, "query key sets must start at 0 and not decrease");
        for (uint32_t q = 0; q < nq; ++q)
            if (lims[q + 1] - lims[q] > PQV_KEY_SET_MAX) return fail(PQV_ERR_INVALID, "a query key set takes at most 1024 values");
        for (uint32_t q = 0; q < nq; ++q)
            for (uint64_t i = lims[q] + 1; i < lims[q + 1]; ++i)
                if (!(vals[i - 1] < vals[i])) return fail(PQV_ERR_INVALID, "query key sets must be strictly ascending");
    }
    return PQV_OK;
}
// (descriptor_checked: the caller made filter_descriptor_checks itself, with checks of its own behind them)
static int filtered_view(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *f, uint32_t nq, const pqv_row_mask *mask,
                         bool host, SearchRequest &mv, bool descriptor_checked = false) {
    if (!descriptor_checked) { if (int rc = filter_descriptor_checks(f, nq, host)) return rc; }
    if (int rc = keyed_view(s, keys, f->a, nq, mask, mv)) return rc;
    if (f->kind == PQV_KEY_EQ) {
        (host ? mv.rows.h_qkeys : mv.rows.d_qkeys) = static_cast<const int64_t *>(f->a);
    } else {
        mv.rows.kind = f->kind;
        if (host) { mv.rows.h_a = f->a; mv.rows.h_b = f->b; }
        else { mv.rows.d_a = f->a; mv.rows.d_b = f->b; }
    }
    return PQV_OK;
}
extern "C" int pqv_topk_filtered(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                                 const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates,
                                 int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = filtered_view(s, keys, filter, nq, mask, true, mv)) return rc;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates, &mv);
    });
}
extern "C" int pqv_topk_filtered_device(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                                        const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric,
                                        int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                                        void *d_tie_flags, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = filtered_view(s, keys, filter, nq, mask, false, mv)) return rc;
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, d_tie_flags, hip_stream, &mv);
    });
}
// ---- expanding filtered top-k (pqv.h: pqv_topk_expand) ---------------------------------------------------------------------
// The checks of both forms up to the view, in the contract's order; nothing is dereferenced before the NULL checks.
static int expand_view(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask, uint32_t nq,
                       uint32_t k, uint32_t nprobe, uint32_t max_nprobe, int metric, bool host, bool flags, SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!keys && !mask) return fail(PQV_ERR_INVALID, "pqv_topk_expand needs a row mask or row keys");
    if (!keys && filter) return fail(PQV_ERR_INVALID, "a key filter needs row keys");
    if (keys && !filter) return fail(PQV_ERR_INVALID, "filter must not be NULL");
    if (keys) { if (int rc = filter_descriptor_checks(filter, nq, host)) return rc; }
    if (max_nprobe < nprobe) return fail(PQV_ERR_INVALID, "max_nprobe must be >= nprobe");
    if (keys) { if (int rc = filtered_view(s, keys, filter, nq, mask, host, mv, true)) return rc; }
    else if (int rc = mask_view(s, mask, mv)) return rc;
    if (int rc = validate_topk(s, k, nprobe, metric)) return rc;
    if (s->n_files) return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_expand does not take table searchers");
    if (metric == PQV_DOT) return fail(PQV_ERR_UNSUPPORTED, "PQV_DOT is not supported by pqv_topk_expand");
    // (the host form always carries the runner-up entry its tie replay needs)
    if (k > (flags ? 1023u : 1024u) || probe_count(s, max_nprobe) > 1024)
        return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_expand takes k <= 1024 (1023 with tie flags) and at most 1024 probed lists per query");
    mv.expand.max_nprobe = max_nprobe;
    return PQV_OK;
}
extern "C" int pqv_topk_expand(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                               const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t max_nprobe,
                               int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates,
                               uint32_t *nprobe_used) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = expand_view(s, keys, filter, mask, nq, k, nprobe, max_nprobe, metric, true, true, mv)) return rc;
        mv.expand.h_used = nprobe_used;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, 0, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates, &mv);
    });
}
extern "C" int pqv_topk_expand_device(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                                      const void *d_queries, uint32_t nq, uint32_t k, uint32_t nprobe, uint32_t max_nprobe, int metric,
                                      int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates,
                                      void *d_nprobe_used, void *d_tie_flags, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = expand_view(s, keys, filter, mask, nq, k, nprobe, max_nprobe, metric, false, d_tie_flags != nullptr, mv)) return rc;
        mv.expand.d_used = static_cast<uint32_t *>(d_nprobe_used);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, 0, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, d_tie_flags, hip_stream, &mv);
    });
}
// ---- per-query probe depths (pqv.h: pqv_topk_depth) ------------------------------------------------------------------------
// The checks of both forms up to the view, in the contract's order; nothing is dereferenced before the NULL checks.
static int depth_view(const pqv_searcher *s, const pqv_probe_depth *d, uint32_t nq, uint32_t k, uint32_t nprobe, int metric, bool flags,
                      SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!d) return fail(PQV_ERR_INVALID, "depth must not be NULL");
    if (d->max_nprobe < nprobe) return fail(PQV_ERR_INVALID, "max_nprobe must be >= nprobe");
    if (d->kind != PQV_DEPTH_GIVEN && d->kind != PQV_DEPTH_RATIO) return fail(PQV_ERR_INVALID, "unknown depth kind " + std::to_string(d->kind));
    if (d->kind == PQV_DEPTH_GIVEN && nq && !d->depths) return fail(PQV_ERR_INVALID, "depths must not be NULL");
    if (d->kind == PQV_DEPTH_RATIO && !(d->d2_ratio >= 1.0f)) return fail(PQV_ERR_INVALID, "d2_ratio must be >= 1 and not NaN");
    if (int rc = validate_topk(s, k, nprobe, metric)) return rc;
    if (s->n_files) return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_depth does not take table searchers");
    if (metric == PQV_DOT) return fail(PQV_ERR_UNSUPPORTED, "PQV_DOT is not supported by pqv_topk_depth");
    // (the host form always carries the runner-up entry its tie replay needs)
    if (k > (flags ? 1023u : 1024u) || probe_count(s, d->max_nprobe) > 1024)
        return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_depth takes k <= 1024 (1023 with tie flags) and at most 1024 probed lists per query");
    mv.expand.max_nprobe = d->max_nprobe;
    mv.expand.source = d->kind == PQV_DEPTH_GIVEN ? DEPTH_GIVEN : DEPTH_RATIO;
    mv.expand.d2_ratio = d->d2_ratio;
    return PQV_OK;
}
extern "C" int pqv_topk_depth(const pqv_searcher *s, const pqv_probe_depth *depth, const float *queries, uint32_t nq, uint32_t query_len,
                              uint32_t k, uint32_t nprobe, int metric, int sqrt_out, uint32_t *row_idx, float *dist, uint32_t *n_found,
                              uint64_t *n_candidates, uint32_t *nprobe_used) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = depth_view(s, depth, nq, k, nprobe, metric, true, mv)) return rc;
        if (depth->kind == PQV_DEPTH_GIVEN) mv.expand.h_depths = static_cast<const uint32_t *>(depth->depths);
        mv.expand.h_used = nprobe_used;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, 0, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates, &mv);
    });
}
extern "C" int pqv_topk_depth_device(const pqv_searcher *s, const pqv_probe_depth *depth, const void *d_queries, uint32_t nq, uint32_t k,
                                     uint32_t nprobe, int metric, int sqrt_out, void *d_row_idx, void *d_dist, void *d_n_found,
                                     void *d_n_candidates, void *d_nprobe_used, void *d_tie_flags, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = depth_view(s, depth, nq, k, nprobe, metric, d_tie_flags != nullptr, mv)) return rc;
        if (depth->kind == PQV_DEPTH_GIVEN) mv.expand.d_depths = static_cast<const uint32_t *>(depth->depths);
        mv.expand.d_used = static_cast<uint32_t *>(d_nprobe_used);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, 0, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, d_tie_flags, hip_stream, &mv);
    });
}
extern "C" int pqv_range_search_filtered(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_key_filter *filter, const pqv_row_mask *mask,
                                         const float *queries, uint32_t nq, uint32_t query_len, float radius, uint32_t nprobe,
                                         uint64_t max_candidates, uint64_t max_results, int metric, int sqrt_out, uint64_t **lims,
                                         uint32_t **row_idx, float **dist, uint64_t *n_within, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = filtered_view(s, keys, filter, nq, mask, true, mv)) return rc;
        return pqv_range_search_impl(s, queries, nq, query_len, radius, nprobe, max_candidates, max_results, metric, sqrt_out ? 1 : 0, lims,
                                     row_idx, dist, n_within, n_candidates, &mv);
    });
}

// ---- key partitions (pqv.h: pqv_key_partition) ----------------------------------------------------------------------------
// The searcher's list positions with a valid key in (key as i64, row id) order, the distinct values and their runs' offsets
// (kernels.h: launch_partition_*).  Positions index d_ids like a mask's image, so one partition serves every layout and the cosine
// searcher.  Immutable; owner / owner_uid are compared, never read through.
struct pqv_key_partition {
    const pqv_searcher *owner = nullptr;
    uint64_t owner_uid = 0;
    int device = 0;
    int dtype = 0;                     // PQV_COL_I32 / PQV_COL_I64
    uint64_t m = 0, n_keys = 0;
    DevBuf d_pos;                      // [m] u32
    DevBuf d_keys;                     // [n_keys] i64, ascending
    DevBuf d_off;                      // [n_keys + 1] u64
};
// Creation: the gather through d_ids, a sort by row (the positions without a key go behind the m that have one), the keys of those m,
// a stable sort by key, the run boundaries.  Two 8-byte counts come back to the host: m between the sorts, n_keys at the end.
static int key_partition_create_impl(const pqv_searcher *s, const pqv_column *c, void *hip_stream, pqv_key_partition **out) {
    if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
    *out = nullptr;
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!c) return fail(PQV_ERR_INVALID, "column must not be NULL");
    if (s->n_files) return fail(PQV_ERR_UNSUPPORTED, "pqv_key_partition_create does not take table searchers");
    if (c->dtype != PQV_COL_I32 && c->dtype != PQV_COL_I64) return fail(PQV_ERR_INVALID, "key column must be PQV_COL_I32 or PQV_COL_I64");
    const uint64_t corpus_rows = s->corpus ? s->corpus->n : 0;
    if (c->n != corpus_rows)
        return fail(PQV_ERR_INVALID, "column has " + std::to_string(c->n) + " rows, the corpus has " + std::to_string(corpus_rows));
    if (c->device != s->device)
        return fail(PQV_ERR_INVALID, "column is on device " + std::to_string(c->device) + ", the searcher on device " + std::to_string(s->device));
    if (int rc = use_device(s->device)) return rc;
    std::unique_ptr<pqv_key_partition> kp(new (std::nothrow) pqv_key_partition());
    if (!kp) return fail(PQV_ERR_OOM, "host allocation failed");
    kp->owner = s; kp->owner_uid = s->uid; kp->device = s->device; kp->dtype = c->dtype;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    const uint64_t n = s->n;
    size_t tmp_bytes = 0;
    HIP_TRY(pqv::launch_partition_tmp_bytes(n, &tmp_bytes));
    DevBuf d_tmp, d_row[2], d_p[2], d_cnt;
    HIP_TRY(d_tmp.alloc(tmp_bytes));
    for (int i = 0; i < 2; ++i) {
        HIP_TRY(d_row[i].alloc(n * sizeof(uint32_t)));
        HIP_TRY(d_p[i].alloc(n * sizeof(uint32_t)));
    }
    HIP_TRY(d_cnt.alloc(2 * sizeof(unsigned long long)));         // {m, n_keys}
    HIP_TRY(hipMemsetAsync(d_cnt.p, 0, 2 * sizeof(unsigned long long), stream));
    HIP_TRY(pqv::launch_partition_gather(c->d_valid, corpus_rows, s->d_ids.as<uint32_t>(), n, d_row[0].as<uint32_t>(), d_p[0].as<uint32_t>(),
                                         d_cnt.as<unsigned long long>(), stream));
    HIP_TRY(pqv::launch_partition_sort_rows(d_row[0].as<uint32_t>(), d_p[0].as<uint32_t>(), d_row[1].as<uint32_t>(), d_p[1].as<uint32_t>(), n,
                                            d_tmp.p, tmp_bytes, stream));
    unsigned long long h_cnt[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(&h_cnt[0], d_cnt.p, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));
    const uint64_t m = h_cnt[0];
    if (m > n) return fail(PQV_ERR_HIP, "key partition build: more keyed positions than positions");
    kp->m = m;
    HIP_TRY(kp->d_pos.alloc(m * sizeof(uint32_t)));
    if (m) {
        DevBuf d_key[2], d_vals, d_run, d_off;
        for (int i = 0; i < 2; ++i) HIP_TRY(d_key[i].alloc(m * sizeof(int64_t)));
        HIP_TRY(d_vals.alloc(m * sizeof(int64_t)));
        HIP_TRY(d_run.alloc(m * sizeof(uint64_t)));
        HIP_TRY(d_off.alloc((m + 1) * sizeof(uint64_t)));
        HIP_TRY(pqv::launch_partition_keys(c->d_values, static_cast<uint32_t>(column_value_size(c->dtype)), d_row[1].as<uint32_t>(), m,
                                           d_key[0].as<int64_t>(), stream));
        HIP_TRY(pqv::launch_partition_sort_keys(d_key[0].as<int64_t>(), d_p[1].as<uint32_t>(), d_key[1].as<int64_t>(), kp->d_pos.as<uint32_t>(), m,
                                                d_tmp.p, tmp_bytes, stream));
        HIP_TRY(hipMemsetAsync(d_run.p, 0, m * sizeof(uint64_t), stream));
        HIP_TRY(pqv::launch_partition_runs(d_key[1].as<int64_t>(), m, d_vals.as<int64_t>(), d_run.as<uint64_t>(), d_off.as<uint64_t>(),
                                           d_cnt.as<unsigned long long>() + 1, d_tmp.p, tmp_bytes, stream));
        HIP_TRY(hipMemcpyAsync(&h_cnt[1], d_cnt.as<unsigned long long>() + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
        const uint64_t nk = h_cnt[1];
        if (nk == 0 || nk > m) return fail(PQV_ERR_HIP, "key partition build: run count out of range");
        kp->n_keys = nk;
        HIP_TRY(kp->d_keys.alloc(nk * sizeof(int64_t)));
        HIP_TRY(kp->d_off.alloc((nk + 1) * sizeof(uint64_t)));
        HIP_TRY(hipMemcpyAsync(kp->d_keys.p, d_vals.p, nk * sizeof(int64_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipMemcpyAsync(kp->d_off.p, d_off.p, (nk + 1) * sizeof(uint64_t), hipMemcpyDeviceToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));      // (the scratch is released at scope exit)
    } else {
        HIP_TRY(kp->d_keys.alloc(0));
        HIP_TRY(kp->d_off.alloc(sizeof(uint64_t)));
        HIP_TRY(hipMemsetAsync(kp->d_off.p, 0, sizeof(uint64_t), stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    *out = kp.release();
    return PQV_OK;
}
extern "C" int pqv_key_partition_create(const pqv_searcher *s, const pqv_column *column, void *hip_stream, pqv_key_partition **out) {
    return guard([&] { return key_partition_create_impl(s, column, hip_stream, out); });
}
extern "C" uint64_t pqv_key_partition_rows(const pqv_key_partition *p) { return p ? p->m : 0; }
extern "C" uint64_t pqv_key_partition_n_keys(const pqv_key_partition *p) { return p ? p->n_keys : 0; }
extern "C" int pqv_key_partition_dtype(const pqv_key_partition *p) { return p ? p->dtype : -1; }
static int key_partition_keys_impl(const pqv_key_partition *p, int64_t *keys, uint64_t *counts, uint64_t n) {
    if (!p) return fail(PQV_ERR_INVALID, "key partition must not be NULL");
    n = std::min<uint64_t>(n, p->n_keys);
    if (n == 0 || (!keys && !counts)) return PQV_OK;
    if (int rc = use_device(p->device)) return rc;
    if (keys) HIP_TRY(hipMemcpy(keys, p->d_keys.p, n * sizeof(int64_t), hipMemcpyDeviceToHost));
    if (counts) {
        std::vector<uint64_t> off;
        try { off.resize(n + 1); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
        HIP_TRY(hipMemcpy(off.data(), p->d_off.p, (n + 1) * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (uint64_t i = 0; i < n; ++i) counts[i] = off[i + 1] - off[i];
    }
    return PQV_OK;
}
extern "C" int pqv_key_partition_keys(const pqv_key_partition *p, int64_t *keys, uint64_t *counts, uint64_t n) {
    return guard([&] { return key_partition_keys_impl(p, keys, counts, n); });
}
extern "C" void pqv_key_partition_free(pqv_key_partition *p) {
    if (!p) return;
    (void)hipSetDevice(p->device);
    delete p;
}

// The checks of every partition entry point, in the contract's order: every NULL and zero check before a handle is read.
// group_size: a grouped call's (gk is then one of its handles), else nullptr; query_len: a host form's; limit: the entry's own bound
// on its lists, k (* group_size) <= 1024 -- nullptr for the range call, which has no k and passes 1.
static int partition_checks(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *f, const pqv_row_keys *gk,
                            const uint32_t *group_size, const pqv_row_mask *mask, uint32_t nq, uint32_t k, int metric, bool host,
                            uint32_t query_len, const char *limit) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!part) return fail(PQV_ERR_INVALID, "key partition must not be NULL");
    if (group_size && !gk) return fail(PQV_ERR_INVALID, "row keys must not be NULL");
    if (int rc = filter_descriptor_checks(f, nq, host)) return rc;
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (group_size && *group_size == 0) return fail(PQV_ERR_INVALID, "group_size must be > 0");
    if (part->owner != s || part->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "key partition belongs to another searcher");
    if (group_size && (gk->owner != s || gk->owner_uid != s->uid)) return fail(PQV_ERR_INVALID, "row keys belong to another searcher");
    if (mask && (mask->owner != s || mask->owner_uid != s->uid)) return fail(PQV_ERR_INVALID, "row mask belongs to another searcher");
    if (int rc = validate_topk(s, k, 1, metric)) return rc;
    if (host && query_len != s->dim)
        return fail(PQV_ERR_INVALID, "Query dimension mismatch: expected " + std::to_string(s->dim) + ", got " + std::to_string(query_len));
    if (group_size && metric == PQV_DOT) return fail(PQV_ERR_UNSUPPORTED, "PQV_DOT is not supported by keyed and distinct calls");
    if (limit && static_cast<uint64_t>(k) * (group_size ? *group_size : 1u) > 1024) return fail(PQV_ERR_UNSUPPORTED, limit);
    return PQV_OK;
}
// blocks per query of partition_stream_kernel: the grid cannot follow span lengths only the device knows, so it comes from the batch
// (about 2048 blocks fill the chip), the partition (a block's turn covers 256 positions: no more blocks than turns over ALL of it)
// and k (the fold reads B * 4 * k entries per query)
static uint32_t partition_blocks(const pqv_searcher *s, uint32_t nq, uint32_t k, uint64_t m) {
    if (s->opt.partition_blocks) return s->opt.partition_blocks;
    uint64_t b = (2048 + static_cast<uint64_t>(nq) - 1) / std::max<uint32_t>(1, nq);
    b = std::min<uint64_t>(b, (m + 255) / 256);
    b = std::min<uint64_t>(b, std::max<uint32_t>(1, 4096 / k));
    return static_cast<uint32_t>(std::max<uint64_t>(1, b));
}
// The walk stage of every partition body.  A call runs in pieces of at most PARTITION_GRID_Q queries (the grid's y): size() sizes,
// once, the scratch that does not depend on the piece; launch() pads a piece's queries where the stored rows are padded, launches
// the span kernel and fills the arguments of the walk that follows -- StreamArgs' common fields (the caller adds k,
// blocks_per_list and its outputs) and all of PartitionArgs.  `s`: the searcher whose rows are read (the call's, or its cosine
// searcher).  Nothing is counted here: launch() is one launch, two where padded().
constexpr uint32_t PARTITION_GRID_Q = 32768;
struct RowMap { const uint32_t *map; uint64_t len; };      // a searcher's row -> list position map (ensure_row_map)
struct PartitionWalk {
    const pqv_searcher *s;
    Scratch &sc;
    const pqv_key_partition *part;
    uint32_t kind;
    const uint64_t *bits;
    int metric;
    hipStream_t stream;
    uint32_t piece = 0;
    // kind SLICE_ROWS (part nullptr): the sequences are a candidate-list call's own slices -- no span kernel, launch_rows_at
    RowMap map{};
    const uint64_t *lims0 = nullptr;    // ... its score form: the lims word of the call's first query (RowsArgs::lims0)

    uint32_t span_w() const { return kind == PQV_KEY_IN ? PQV_KEY_SET_MAX : 1u; }      // span slots per query
    bool padded() const { return s->sdim != s->dim; }
    int size(uint32_t nq) {
        piece = std::min<uint32_t>(nq, PARTITION_GRID_Q);
        if (kind != SLICE_ROWS) {
            HIP_TRY(sc.s_pt_beg.ensure(static_cast<size_t>(piece) * span_w() * sizeof(uint32_t)));
            if (kind == PQV_KEY_IN) {
                HIP_TRY(sc.s_pt_end.ensure(static_cast<size_t>(piece) * span_w() * sizeof(uint32_t)));
                HIP_TRY(sc.s_pt_nspan.ensure(static_cast<size_t>(piece) * sizeof(uint32_t)));
            }
            HIP_TRY(sc.s_ncand.ensure(static_cast<size_t>(piece) * sizeof(uint64_t)));
        }
        if (padded()) HIP_TRY(sc.s_qpad.ensure(static_cast<size_t>(piece) * s->sdim * sizeof(float)));
        return PQV_OK;
    }
    // the b queries at dq, padded where the stored rows are, and StreamArgs' common fields
    int stream_args(const float *dq, uint32_t b, pqv::StreamArgs &ra) const {
        using namespace pqv;
        if (padded()) {      // (the stored rows are zero-padded: the queries that meet them too)
            HIP_TRY(launch_pad_rows(dq, nullptr, b, s->dim, s->sdim, sc.s_qpad.as<float>(), stream));
            dq = sc.s_qpad.as<float>();
        }
        ra = StreamArgs{};
        ra.mat = s->d_mat; ra.row_of = s->d_row_of;
        ra.queries = dq; ra.nq = b; ra.nprobe = 1; ra.dim = s->sdim;
        ra.rows_per_block = 256; ra.max_pos = ~0ull; ra.metric = metric;
        return PQV_OK;
    }
    // the b queries at dq, with d_a / d_b as the span kernel indexes them from this piece's first query
    int launch(const float *dq, uint32_t b, const void *d_a, const void *d_b, uint64_t *d_n_cand_out, pqv::StreamArgs &ra,
               pqv::PartitionArgs &pa) const {
        using namespace pqv;
        if (int rc = stream_args(dq, b, ra)) return rc;
        PartitionSpanArgs sp{};
        sp.keys = part->d_keys.as<int64_t>(); sp.key_off = part->d_off.as<uint64_t>(); sp.n_keys = part->n_keys;
        sp.nq = b; sp.kind = kind; sp.a = d_a; sp.b = d_b;
        sp.span_beg = sc.s_pt_beg.as<uint32_t>(); sp.span_end = sc.s_pt_end.as<uint32_t>(); sp.n_span = sc.s_pt_nspan.as<uint32_t>();
        sp.n_cand = sc.s_ncand.as<uint64_t>(); sp.n_cand_out = d_n_cand_out;
        sp.stats = s->d_stats.as<unsigned long long>();
        HIP_TRY(launch_partition_span(sp, stream));
        pa = PartitionArgs{};
        pa.pos = part->d_pos.as<uint32_t>(); pa.span_beg = sp.span_beg; pa.span_end = sp.span_end; pa.n_span = sp.n_span;
        pa.n_cand = sp.n_cand; pa.kind = kind; pa.bits = bits; pa.stats = sp.stats;
        return PQV_OK;
    }
    // the piece [q0, q0 + b) of a call whose queries and a / b are whole DEVICE arrays: every kind's a is indexed by query -- an IN
    // filter's lims hold offsets into ALL of b -- so a piece takes a + q0 and, but for a RANGE filter's, b as it is.  o: the
    // piece's output block (TopkOut::at), whose n_cand the span kernel writes.
    int launch_at(uint32_t q0, uint32_t b, const float *d_queries, const void *d_a, const void *d_b, const TopkOut &o, pqv::StreamArgs &ra,
                  pqv::PartitionArgs &pa) const {
        const size_t off = static_cast<size_t>(q0) * 8;
        return launch(d_queries + static_cast<size_t>(q0) * s->dim, b, static_cast<const char *>(d_a) + off,
                      kind == PQV_KEY_RANGE ? static_cast<const void *>(static_cast<const char *>(d_b) + off) : d_b, o.n_cand, ra, pa);
    }
    // SLICE_ROWS: the same piece of a candidate-list call -- d_lims indexed from the piece's first query, d_rows whole (lims hold
    // offsets into all of it); nothing is launched beside the padding, the walk's kernel reads the slices itself
    int launch_rows_at(uint32_t q0, uint32_t b, const float *d_queries, const void *d_lims, const void *d_rows, const TopkOut &o,
                       pqv::StreamArgs &ra, pqv::RowsArgs &wa) const {
        if (int rc = stream_args(d_queries + static_cast<size_t>(q0) * s->dim, b, ra)) return rc;
        wa = pqv::RowsArgs{};
        wa.lims = static_cast<const uint64_t *>(d_lims) + q0; wa.cand_rows = static_cast<const uint32_t *>(d_rows);
        wa.map = map.map; wa.map_len = map.len; wa.bits = bits; wa.stats = s->d_stats.as<unsigned long long>();
        wa.n_cand_out = o.n_cand; wa.lims0 = lims0;
        return PQV_OK;
    }
};
// A device form behind its checks: the lock, the lane, body(searcher, scratch, queries, metric, sqrt_out) and the queries counted.
// PQV_COSINE: n(q) into this searcher's lane, then the L2 body on the cosine searcher (sqrt_out 2) under ITS lock and lane, taken
// second and released first.
template <class Body>
static int partition_device_call(const pqv_searcher *s, const float *d_queries, uint32_t nq, int metric, int sqrt_out, hipStream_t stream, Body body) {
    std::lock_guard<std::mutex> lock(s->mu);
    Lane lane;
    if (metric == PQV_COSINE) {
        if (int rc = cosine_queries_device(s, d_queries, nq, stream, lane)) return rc;
        const pqv_searcher *cs = s->cos.get();
        std::lock_guard<std::mutex> cos_lock(cs->mu);
        Lane cos_lane;
        if (int rc = cos_lane.acquire(cs, stream)) return rc;
        if (int rc = body(cs, *cos_lane, lane->s_qcos.as<float>(), PQV_L2SQ_REF4, 2)) return rc;
        cs->counters.queries += nq;
        if (int rc = cos_lane.release()) return rc;
        return lane.release();
    }
    if (int rc = lane.acquire(s, stream)) return rc;
    if (int rc = body(s, *lane, d_queries, metric, sqrt_out)) return rc;
    s->counters.queries += nq;
    return lane.release();
}
// the descriptor's host arrays as a request, for the sub-batches' (pieces') slices: upload_query_filter
static SearchRequest partition_request(const pqv_key_filter *f) {
    SearchRequest rq{};
    rq.rows.kind = f->kind;
    if (f->kind == PQV_KEY_EQ) rq.rows.h_qkeys = static_cast<const int64_t *>(f->a);
    else { rq.rows.h_a = f->a; rq.rows.h_b = f->b; }
    return rq;
}
// The outputs of a host form of the partition family (topk_partition_host_body) on a lane: `host`, the caller's arrays (rows and
// dist k * m per query; none at all: the score form, which brings its distances back itself), as the list host_batches sizes and
// copies back, and as the block over the same scratch buffers that a sub-batch's kernels write.  n_candidates comes back through
// s_out: the walk stage uses s_ncand itself.  A grouped call's keys are always written (group_key NULL: sized, not copied), its rows
// per group where the caller takes them.
struct PartitionHostOuts {
    TopkOut host; uint32_t k; uint64_t km; bool grouped;
    bool rows_per_group() const { return grouped && host.group_rows; }
    std::vector<BatchOut> batch(Scratch &sc) const {
        if (!host.dist) return {};
        std::vector<BatchOut> outs = {{&sc.s_rows, km * sizeof(uint32_t), host.rows}, {&sc.s_dist, km * sizeof(float), host.dist},
                                      {&sc.s_nfound, sizeof(uint32_t), host.n_found}, {&sc.s_out, sizeof(uint64_t), host.n_cand}};
        if (grouped) outs.push_back({&sc.s_grp_out, k * sizeof(int64_t), host.group_key});
        if (rows_per_group()) outs.push_back({&sc.s_grows_out, k * sizeof(uint32_t), host.group_rows});
        return outs;
    }
    TopkOut dev(Scratch &sc) const {      // (once host_batches has sized them)
        if (!host.dist) return TopkOut{};
        return TopkOut{sc.s_rows.as<uint32_t>(), sc.s_dist.as<float>(), sc.s_nfound.as<uint32_t>(), sc.s_out.as<uint64_t>(),
                       grouped ? sc.s_grp_out.as<int64_t>() : nullptr, rows_per_group() ? sc.s_grows_out.as<uint32_t>() : nullptr};
    }
};
// The host form of the partition top-k calls and the candidate-list calls: PQV_COSINE's n(q), the lane, sub-batches of queries
// through it (rq's per-query slices -- a filter's, or the candidate lists -- uploaded as pqv_topk_filtered uploads a filter's; m:
// the positions partition_blocks sizes the grid by), enqueue(s, sc, bits, d_a, d_b, b, metric, sqrt_out, out) -- the device body on a
// sub-batch's scratch, out: outs.dev(sc) -- and outs.batch(sc) back.  The sub-batch is bounded so the scratch stays under ~1 GiB: per
// query the B * 4 per-wave lists of k_lists entries, list_bytes in all passes' widest, the padded query, and out_bytes of outputs and
// filter slice.
template <class Enqueue>
static int topk_partition_host_body(const pqv_searcher *s, uint64_t m, const SearchRequest &rq, const pqv_row_mask *mask,
                                    const float *queries, uint32_t nq, uint32_t k_lists, int metric, int sqrt_out, uint64_t list_bytes,
                                    uint64_t out_bytes, const PartitionHostOuts &outs, Enqueue enqueue) {
    std::vector<float> nq_host;
    if (int rc = cosine_queries_host(s, queries, nq, metric, sqrt_out, nq_host)) return rc;
    const uint64_t *bits = mask ? mask->d_bits.as<uint64_t>() : nullptr;
    std::lock_guard<std::mutex> lock(s->mu);
    Lane lane;
    if (int rc = lane.acquire(s, s->stream)) return rc;
    Scratch &sc = *lane;
    const uint32_t B = partition_blocks(s, std::min<uint32_t>(nq, 1024), k_lists, m);
    const uint64_t per_query = static_cast<uint64_t>(B) * 4 * list_bytes + static_cast<uint64_t>(s->sdim) * 8 + out_bytes;
    const uint32_t batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(std::min<uint32_t>(nq, PARTITION_GRID_Q), (1ull << 30) / per_query)));
    if (int rc = host_batches(
            s, sc, queries, nq, batch, &rq, nullptr, outs.batch(sc),
            [&](uint32_t b, SearchRequest *brq) {
                return enqueue(s, sc, bits, brq->d_filter_a(), brq->d_filter_b(), b, metric, sqrt_out, outs.dev(sc));
            },
            [](uint32_t, uint32_t) { return static_cast<int>(PQV_OK); }))      // (no host step)
        return rc;
    return lane.release();
}

// ---- top-k over a key partition (pqv.h: pqv_topk_partition) ----------------------------------------------------------------------
// The fold of a piece's per-wave lists (ra: the walk's arguments, n_part lists of ra.k entries per query) into the piece's output
// block o: merge_kernel, PQV_DOT: dot_merge_kernel.
static int partition_fold(const pqv_searcher *s, const pqv::StreamArgs &ra, uint32_t n_part, int metric, int sqrt_out, const TopkOut &o,
                          hipStream_t stream) {
    using namespace pqv;
    const uint32_t k = ra.k;
    MergeArgs fm{};
    fm.part_keys = ra.part_keys; fm.part_vals = ra.part_vals;
    fm.nq = ra.nq; fm.n_part = n_part; fm.k_part = k; fm.k = k;
    fm.ids = s->d_final_ids; fm.row_idx = o.rows; fm.dist = o.dist; fm.n_found = o.n_found;
    fm.sqrt_out = sqrt_out; fm.k_out = k;
    if (metric == PQV_DOT) HIP_TRY(launch_dot_merge(fm, stream));
    else HIP_TRY(launch_merge_final(fm, stream));
    return PQV_OK;
}
// Enqueue span -> stream -> fold for the queries [0, nq) on `stream`, in PartitionWalk's pieces.  a / b: the descriptor's DEVICE arrays;
// out: the call's outputs.
static int enqueue_partition(const pqv_searcher *s, Scratch &sc, const pqv_key_partition *part, uint32_t kind, const void *d_a, const void *d_b,
                             const uint64_t *bits, const float *d_queries, uint32_t nq, uint32_t k, int metric, int sqrt_out,
                             const TopkOut &out, hipStream_t stream) {
    using namespace pqv;
    PartitionWalk w{s, sc, part, kind, bits, metric, stream};
    if (int rc = w.size(nq)) return rc;
    const uint32_t B = partition_blocks(s, w.piece, k, part->m);
    const uint32_t n_part = B * waves_per_block();
    HIP_TRY(sc.s_part_keys.ensure((static_cast<size_t>(w.piece) * n_part * k + 4) * sizeof(uint64_t)));
    HIP_TRY(sc.s_part_vals.ensure((static_cast<size_t>(w.piece) * n_part * k + 4) * sizeof(uint32_t)));
    for (uint32_t q0 = 0; q0 < nq; q0 += w.piece) {
        const uint32_t b = std::min<uint32_t>(w.piece, nq - q0);
        const TopkOut o = out.at(q0, k, k);
        StreamArgs ra;
        PartitionArgs pa;
        if (int rc = w.launch_at(q0, b, d_queries, d_a, d_b, o, ra, pa)) return rc;
        ra.k = k; ra.blocks_per_list = B;
        ra.part_keys = sc.s_part_keys.as<uint64_t>(); ra.part_vals = sc.s_part_vals.as<uint32_t>();
        HIP_TRY(launch_partition_stream(ra, pa, stream));
        if (int rc = partition_fold(s, ra, n_part, metric, sqrt_out, o, stream)) return rc;
        s->counters.kernel_launches += 3;
    }
    return PQV_OK;
}
extern "C" int pqv_topk_partition_device(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *filter,
                                         const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k, int metric, int sqrt_out,
                                         void *d_row_idx, void *d_dist, void *d_n_found, void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        if (int rc = partition_checks(s, part, filter, nullptr, nullptr, mask, nq, k, metric, false, 0, "pqv_topk_partition takes k <= 1024")) return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!d_queries || !d_row_idx || !d_dist) return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
        const uint64_t *bits = mask ? mask->d_bits.as<uint64_t>() : nullptr;
        const TopkOut out{static_cast<uint32_t *>(d_row_idx), static_cast<float *>(d_dist), static_cast<uint32_t *>(d_n_found),
                          static_cast<uint64_t *>(d_n_candidates)};
        return partition_device_call(s, static_cast<const float *>(d_queries), nq, metric, sqrt_out ? 1 : 0, stream,
                                     [&](const pqv_searcher *bs, Scratch &sc, const float *q, int mt, int so) {
                                         return enqueue_partition(bs, sc, part, filter->kind, filter->a, filter->b, bits, q, nq, k, mt, so, out, stream);
                                     });
    });
}
extern "C" int pqv_topk_partition(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *filter, const pqv_row_mask *mask,
                                  const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, int metric, int sqrt_out,
                                  uint32_t *row_idx, float *dist, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        if (int rc = partition_checks(s, part, filter, nullptr, nullptr, mask, nq, k, metric, true, query_len, "pqv_topk_partition takes k <= 1024")) return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!queries || !row_idx || !dist) return fail(PQV_ERR_INVALID, "queries/row_idx/dist must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        // (per list entry 12 B; beside the lists the rows, distances and n_found / n_candidates, and an IN slice)
        return topk_partition_host_body(
            s, part->m, partition_request(filter), mask, queries, nq, k, metric, sqrt_out ? 1 : 0, 12ull * k, 12ull * k + 8 * PQV_KEY_SET_MAX,
            PartitionHostOuts{{row_idx, dist, n_found, n_candidates}, k, k, false},
            [&](const pqv_searcher *bs, Scratch &sc, const uint64_t *bits, const void *d_a, const void *d_b, uint32_t b, int mt, int so,
                const TopkOut &out) {
                return enqueue_partition(bs, sc, part, filter->kind, d_a, d_b, bits, sc.s_queries.as<float>(), b, k, mt, so, out, bs->stream);
            });
    });
}

// ---- candidate lists (pqv.h: pqv_topk_rows, pqv_score_rows) ------------------------------------------------------------------------
// The partition walk stage over sequences the caller wrote: query q's is cand_rows[lims[q] .. lims[q + 1]), a position's list
// position comes from the searcher's row map.  One body for the four entry points: k == 0 is the score form, whose d_dist takes a
// distance per candidate instead of the fold's k per query.
// The row map of `s`, made by its first candidate-list call under s->mu: 4 bytes per corpus row, one fill and one scatter over
// d_ids on the searcher's stream, waited for -- later calls run on any stream.
static int ensure_row_map(const pqv_searcher *s, RowMap &out) {
    std::lock_guard<std::mutex> lock(s->mu);
    if (!s->row_map_done) {
        const uint64_t rows = s->corpus ? s->corpus->n : 0;
        HIP_TRY(s->d_row_map.alloc(rows * sizeof(uint32_t)));
        HIP_TRY(pqv::launch_row_map(s->d_ids.as<uint32_t>(), s->n, s->d_row_map.as<uint32_t>(), rows, s->stream));
        HIP_TRY(hipStreamSynchronize(s->stream));
        s->row_map_len = rows;
        s->row_map_done = true;
        s->counters.kernel_launches += 1;
    }
    out = RowMap{s->d_row_map.as<uint32_t>(), s->row_map_len};
    return PQV_OK;
}
// The checks of the four entry points up to the query length, in the contract's order, all before any device use.  k: a top-k
// form's, else nullptr; host: lims / cand_rows are host arrays -- cand_rows may then be NULL where every slice is empty, and the
// slices are checked; who: the entry point's name for the table refusal.
static int rows_checks(const pqv_searcher *s, const void *lims, const void *cand_rows, const pqv_row_mask *mask, uint32_t nq, const uint32_t *k,
                       int metric, bool host, uint32_t query_len, const char *who) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!lims) return fail(PQV_ERR_INVALID, "lims must not be NULL");
    const uint64_t *hl = host ? static_cast<const uint64_t *>(lims) : nullptr;
    bool any = !host;
    for (uint32_t q = 0; q < nq && !any; ++q) any = hl[q + 1] != hl[q];
    if (any && !cand_rows) return fail(PQV_ERR_INVALID, "cand_rows must not be NULL");
    if (k && *k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (host) {
        for (uint32_t q = 0; q < nq; ++q)
            if (hl[q + 1] < hl[q]) return fail(PQV_ERR_INVALID, "lims must not decrease");
        for (uint32_t q = 0; q < nq; ++q)
            if (hl[q + 1] - hl[q] > 0xFFFFFFFFull) return fail(PQV_ERR_INVALID, "a candidate list holds at most 2^32 - 1 rows");
    }
    if (mask && (mask->owner != s || mask->owner_uid != s->uid)) return fail(PQV_ERR_INVALID, "row mask belongs to another searcher");
    if (s->n_files) return fail(PQV_ERR_UNSUPPORTED, std::string(who) + " does not take table searchers");
    if (int rc = validate_topk(s, 1, 1, metric)) return rc;
    if (host && query_len != s->dim)
        return fail(PQV_ERR_INVALID, "Query dimension mismatch: expected " + std::to_string(s->dim) + ", got " + std::to_string(query_len));
    return PQV_OK;
}
// Enqueue walk (-> fold) for the queries [0, nq) on `stream`, in PartitionWalk's pieces.  d_lims / d_rows: DEVICE arrays; lims0: the
// device word the score form's output offsets are taken from; out: the call's outputs (k == 0: dist alone, a distance per candidate).
static int enqueue_rows(const pqv_searcher *s, Scratch &sc, const RowMap &map, const void *d_lims, const void *d_rows, const uint64_t *lims0,
                        const uint64_t *bits, const float *d_queries, uint32_t nq, uint32_t k, int metric, int sqrt_out, const TopkOut &out,
                        hipStream_t stream) {
    using namespace pqv;
    PartitionWalk w{s, sc, nullptr, SLICE_ROWS, bits, metric, stream};
    w.map = map; w.lims0 = lims0;
    if (int rc = w.size(nq)) return rc;
    const uint32_t B = partition_blocks(s, w.piece, std::max<uint32_t>(1, k), s->n);
    const uint32_t n_part = B * waves_per_block();
    if (k) {
        HIP_TRY(sc.s_part_keys.ensure((static_cast<size_t>(w.piece) * n_part * k + 4) * sizeof(uint64_t)));
        HIP_TRY(sc.s_part_vals.ensure((static_cast<size_t>(w.piece) * n_part * k + 4) * sizeof(uint32_t)));
    }
    for (uint32_t q0 = 0; q0 < nq; q0 += w.piece) {
        const uint32_t b = std::min<uint32_t>(w.piece, nq - q0);
        const TopkOut o = out.at(q0, k, k);
        StreamArgs ra;
        RowsArgs wa;
        if (int rc = w.launch_rows_at(q0, b, d_queries, d_lims, d_rows, o, ra, wa)) return rc;
        ra.k = k; ra.blocks_per_list = B;
        if (k) {
            ra.part_keys = sc.s_part_keys.as<uint64_t>(); ra.part_vals = sc.s_part_vals.as<uint32_t>();
            HIP_TRY(launch_rows_stream(ra, wa, stream));
            if (int rc = partition_fold(s, ra, n_part, metric, sqrt_out, o, stream)) return rc;
            s->counters.kernel_launches += 2;
        } else {
            ra.out_f32 = o.dist; ra.sqrt_out = sqrt_out;
            HIP_TRY(launch_rows_score(ra, wa, stream));
            s->counters.kernel_launches += 1;
        }
    }
    return PQV_OK;
}
// the device forms behind their checks (k == 0: scores)
static int rows_device_impl(const pqv_searcher *s, const void *d_lims, const void *d_rows, const pqv_row_mask *mask, const void *d_queries,
                            uint32_t nq, uint32_t k, int metric, int sqrt_out, const TopkOut &out, void *hip_stream) {
    if (nq == 0) return PQV_OK;
    if (!d_queries) return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
    if (int rc = use_device(s->device)) return rc;
    RowMap map{};
    if (int rc = ensure_row_map(s, map)) return rc;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
    const uint64_t *bits = mask ? mask->d_bits.as<uint64_t>() : nullptr;
    return partition_device_call(s, static_cast<const float *>(d_queries), nq, metric, sqrt_out ? 1 : 0, stream,
                                 [&](const pqv_searcher *bs, Scratch &sc, const float *q, int mt, int so) {
                                     return enqueue_rows(bs, sc, map, d_lims, d_rows, static_cast<const uint64_t *>(d_lims), bits, q, nq, k, mt, so,
                                                         out, stream);
                                 });
}
extern "C" int pqv_topk_rows_device(const pqv_searcher *s, const void *d_lims, const void *d_cand_rows, const pqv_row_mask *mask,
                                    const void *d_queries, uint32_t nq, uint32_t k, int metric, int sqrt_out, void *d_row_idx, void *d_dist,
                                    void *d_n_found, void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        if (int rc = rows_checks(s, d_lims, d_cand_rows, mask, nq, &k, metric, false, 0, "pqv_topk_rows")) return rc;
        if (nq && (!d_row_idx || !d_dist)) return fail(PQV_ERR_INVALID, "row_idx/dist must not be NULL");
        if (k > 1024) return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_rows takes k <= 1024");
        const TopkOut out{static_cast<uint32_t *>(d_row_idx), static_cast<float *>(d_dist), static_cast<uint32_t *>(d_n_found),
                          static_cast<uint64_t *>(d_n_candidates)};
        return rows_device_impl(s, d_lims, d_cand_rows, mask, d_queries, nq, k, metric, sqrt_out, out, hip_stream);
    });
}
extern "C" int pqv_score_rows_device(const pqv_searcher *s, const void *d_lims, const void *d_cand_rows, const pqv_row_mask *mask,
                                     const void *d_queries, uint32_t nq, int metric, int sqrt_out, void *d_dist, void *hip_stream) {
    return guard([&] {
        if (int rc = rows_checks(s, d_lims, d_cand_rows, mask, nq, nullptr, metric, false, 0, "pqv_score_rows")) return rc;
        if (nq && !d_dist) return fail(PQV_ERR_INVALID, "dist must not be NULL");
        return rows_device_impl(s, d_lims, d_cand_rows, mask, d_queries, nq, 0, metric, sqrt_out, TopkOut{nullptr, static_cast<float *>(d_dist)},
                                hip_stream);
    });
}
// the host forms' request: the slices travel through host_batches as an IN filter's do
static SearchRequest rows_request(const uint64_t *lims, const uint32_t *cand_rows) {
    SearchRequest rq{};
    rq.rows.kind = SLICE_ROWS; rq.rows.h_a = lims; rq.rows.h_b = cand_rows;
    return rq;
}
extern "C" int pqv_topk_rows(const pqv_searcher *s, const uint64_t *lims, const uint32_t *cand_rows, const pqv_row_mask *mask,
                             const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, int metric, int sqrt_out, uint32_t *row_idx,
                             float *dist, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        if (int rc = rows_checks(s, lims, cand_rows, mask, nq, &k, metric, true, query_len, "pqv_topk_rows")) return rc;
        if (nq && (!row_idx || !dist)) return fail(PQV_ERR_INVALID, "row_idx/dist must not be NULL");
        if (k > 1024) return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_rows takes k <= 1024");
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!queries) return fail(PQV_ERR_INVALID, "queries must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        RowMap map{};
        if (int rc = ensure_row_map(s, map)) return rc;
        // (per list entry 12 B; beside the lists the rows, distances and n_found / n_candidates; the slices are as long as the caller made them)
        return topk_partition_host_body(
            s, s->n, rows_request(lims, cand_rows), mask, queries, nq, k, metric, sqrt_out ? 1 : 0, 12ull * k, 12ull * k + 12,
            PartitionHostOuts{{row_idx, dist, n_found, n_candidates}, k, k, false},
            [&](const pqv_searcher *bs, Scratch &sc, const uint64_t *bits, const void *d_a, const void *d_b, uint32_t b, int mt, int so,
                const TopkOut &out) {
                return enqueue_rows(bs, sc, map, d_a, d_b, nullptr, bits, sc.s_queries.as<float>(), b, k, mt, so, out, bs->stream);
            });
    });
}
extern "C" int pqv_score_rows(const pqv_searcher *s, const uint64_t *lims, const uint32_t *cand_rows, const pqv_row_mask *mask,
                              const float *queries, uint32_t nq, uint32_t query_len, int metric, int sqrt_out, float *dist) {
    return guard([&] {
        if (int rc = rows_checks(s, lims, cand_rows, mask, nq, nullptr, metric, true, query_len, "pqv_score_rows")) return rc;
        if (nq && lims[nq] != lims[0] && !dist) return fail(PQV_ERR_INVALID, "dist must not be NULL");
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!queries) return fail(PQV_ERR_INVALID, "queries must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        RowMap map{};
        if (int rc = ensure_row_map(s, map)) return rc;
        // a sub-batch's distances come back from s_dist as one run of the caller's array: its slices are consecutive there (the
        // sub-batches arrive in order: q_done is the first query of the one being enqueued)
        uint32_t q_done = 0;
        return topk_partition_host_body(
            s, s->n, rows_request(lims, cand_rows), mask, queries, nq, 1, metric, sqrt_out ? 1 : 0, 0, 8,
            PartitionHostOuts{},
            [&](const pqv_searcher *bs, Scratch &sc, const uint64_t *bits, const void *d_a, const void *d_b, uint32_t b, int mt, int so,
                const TopkOut &) {
                const uint64_t first = lims[q_done], n_vals = lims[q_done + b] - first;
                q_done += b;
                HIP_TRY(sc.s_dist.ensure(static_cast<size_t>(n_vals) * sizeof(float)));
                if (int rc = enqueue_rows(bs, sc, map, d_a, d_b, static_cast<const uint64_t *>(d_a), bits, sc.s_queries.as<float>(), b, 0, mt, so,
                                          TopkOut{nullptr, sc.s_dist.as<float>()}, bs->stream))
                    return rc;
                if (n_vals)
                    HIP_TRY(hipMemcpyAsync(dist + (first - lims[0]), sc.s_dist.p, static_cast<size_t>(n_vals) * sizeof(float), hipMemcpyDeviceToHost,
                                           bs->stream));
                return static_cast<int>(PQV_OK);
            });
    });
}

// ---- MMR selection (pqv.h: pqv_mmr_select, pqv_topk_mmr) ---------------------------------------------------------------------------
// One kernel (mmr_select_kernel) over [nq, n] candidates: the caller's (pqv_mmr_select*), or stage 1's in the lane
// (pqv_topk_mmr*: enqueue_topk with k = fetch_k, a mask as pqv_topk_masked carries it, then the selection on the same stream).
// The checks of the four entry points, in the contract's order, all before any device use.  n: the candidates per query (fetch_k);
// fused: pqv_topk_mmr*, which probes; host: the form that takes its queries from the host.
static int mmr_checks(const pqv_searcher *s, const pqv_row_mask *mask, uint32_t k, uint32_t n, float lambda, bool fused, uint32_t nprobe,
                      int metric, bool host, uint32_t query_len) {
    const char *who = fused ? "pqv_topk_mmr" : "pqv_mmr_select";
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (fused && n < k) return fail(PQV_ERR_INVALID, "fetch_k must be >= k");
    if (!(lambda >= 0.0f && lambda <= 1.0f)) return fail(PQV_ERR_INVALID, "lambda must be in [0, 1]");
    if (n > 1024) return fail(PQV_ERR_UNSUPPORTED, fused ? "pqv_topk_mmr takes fetch_k <= 1024" : "pqv_mmr_select takes n <= 1024");
    if (mask && (mask->owner != s || mask->owner_uid != s->uid)) return fail(PQV_ERR_INVALID, "row mask belongs to another searcher");
    if (s->n_files) return fail(PQV_ERR_UNSUPPORTED, std::string(who) + " does not take table searchers");
    if (int rc = validate_topk(s, k, fused ? nprobe : 1, metric)) return rc;
    if (fused) {
        if (int rc = dot_checks(s, n, nprobe, metric, nullptr)) return rc;
        if (beyond_kernel_lists(s, n, nprobe)) return fail(PQV_ERR_UNSUPPORTED, "pqv_topk_mmr takes min(nprobe, n_clusters) <= 1024");
    }
    if (host && query_len != s->dim)
        return fail(PQV_ERR_INVALID, "Query dimension mismatch: expected " + std::to_string(s->dim) + ", got " + std::to_string(query_len));
    return PQV_OK;
}
// a selection's device arrays: the candidates [nq, n] (nf_in: optional [nq]) and the picks [nq, k] (score, nf: optional)
struct MmrIo {
    const uint32_t *rows; const float *dist; const uint32_t *nf_in;
    uint32_t *o_rows; float *o_dist; float *o_score; uint32_t *o_nf;
};
// the selection launch over the rows of `s` (the call's searcher, or its cosine searcher with sqrt_out 2)
static int enqueue_mmr(const pqv_searcher *s, const RowMap &map, const MmrIo &io, uint32_t nq, uint32_t n, uint32_t k, float lambda, int metric,
                       int sqrt_out, hipStream_t stream) {
    using namespace pqv;
    StreamArgs a{};
    a.mat = s->d_mat; a.row_of = s->d_row_of; a.nq = nq; a.dim = s->sdim; a.metric = metric; a.sqrt_out = sqrt_out;
    MmrArgs ma{};
    ma.cand_rows = io.rows; ma.cand_dist = io.dist; ma.n_found_in = io.nf_in; ma.map = map.map; ma.map_len = map.len;
    ma.n = n; ma.k = k; ma.lambda = lambda;
    ma.row_idx = io.o_rows; ma.dist = io.o_dist; ma.score = io.o_score; ma.n_found = io.o_nf;
    HIP_TRY(launch_mmr_select(a, ma, stream));
    s->counters.kernel_launches += 1;
    return PQV_OK;
}
// The searcher whose rows a selection without queries reads: `s`, or -- PQV_COSINE -- its cosine searcher, made here where this is
// the first cosine call, with the L2 chain over its normalised rows and the halving write-out.
static int mmr_rows_searcher(const pqv_searcher *s, int &metric, int &sqrt_out, const pqv_searcher *&rows) {
    rows = s;
    if (metric != PQV_COSINE) return PQV_OK;
    std::lock_guard<std::mutex> lock(s->mu);
    if (int rc = ensure_cosine(s)) return rc;
    rows = s->cos.get(); metric = PQV_L2SQ_REF4; sqrt_out = 2;
    return PQV_OK;
}
extern "C" int pqv_mmr_select_device(const pqv_searcher *s, const void *d_cand_rows, const void *d_cand_dist, const void *d_n_found_in, uint32_t nq,
                                     uint32_t n, uint32_t k, float lambda, int metric, int sqrt_out, void *d_row_idx, void *d_dist, void *d_score,
                                     void *d_n_found, void *hip_stream) {
    return guard([&] {
        if (int rc = mmr_checks(s, nullptr, k, n, lambda, false, 1, metric, false, 0)) return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (n && (!d_cand_rows || !d_cand_dist)) return fail(PQV_ERR_INVALID, "cand_rows/cand_dist must not be NULL");
        if (!d_row_idx || !d_dist) return fail(PQV_ERR_INVALID, "row_idx/dist must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        RowMap map{};
        if (int rc = ensure_row_map(s, map)) return rc;
        hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
        int mt = metric, so = sqrt_out ? 1 : 0;
        const pqv_searcher *rs = nullptr;
        if (int rc = mmr_rows_searcher(s, mt, so, rs)) return rc;
        const MmrIo io{static_cast<const uint32_t *>(d_cand_rows), static_cast<const float *>(d_cand_dist), static_cast<const uint32_t *>(d_n_found_in),
                       static_cast<uint32_t *>(d_row_idx), static_cast<float *>(d_dist), static_cast<float *>(d_score), static_cast<uint32_t *>(d_n_found)};
        std::lock_guard<std::mutex> lock(rs->mu);
        if (int rc = enqueue_mmr(rs, map, io, nq, n, k, lambda, mt, so, stream)) return rc;
        rs->counters.queries += nq;
        return static_cast<int>(PQV_OK);
    });
}
extern "C" int pqv_mmr_select(const pqv_searcher *s, const uint32_t *cand_rows, const float *cand_dist, const uint32_t *n_found_in, uint32_t nq, uint32_t n,
                              uint32_t k, float lambda, int metric, int sqrt_out, uint32_t *row_idx, float *dist, float *score, uint32_t *n_found) {
    return guard([&] {
        if (int rc = mmr_checks(s, nullptr, k, n, lambda, false, 1, metric, false, 0)) return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (n && (!cand_rows || !cand_dist)) return fail(PQV_ERR_INVALID, "cand_rows/cand_dist must not be NULL");
        if (!row_idx || !dist) return fail(PQV_ERR_INVALID, "row_idx/dist must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        RowMap map{};
        if (int rc = ensure_row_map(s, map)) return rc;
        int mt = metric, so = sqrt_out ? 1 : 0;
        const pqv_searcher *rs = nullptr;
        if (int rc = mmr_rows_searcher(s, mt, so, rs)) return rc;
        std::lock_guard<std::mutex> lock(rs->mu);
        Lane lane;
        if (int rc = lane.acquire(rs, rs->stream)) return rc;
        Scratch &sc = *lane;
        // sub-batches of queries through the lane: per query the candidates in and the picks out and nothing else, so 64 MiB of
        // them already amortise a sub-batch's synchronisation
        const uint64_t per_query = 8ull * n + 12ull * k + 8;
        const uint32_t batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(nq, (1ull << 26) / per_query)));
        const size_t in_w = static_cast<size_t>(n) * sizeof(uint32_t), out_w = static_cast<size_t>(k) * sizeof(uint32_t);
        HIP_TRY(sc.s_mmr_rows.ensure(std::max<size_t>(1, batch * in_w)));
        HIP_TRY(sc.s_mmr_dist.ensure(std::max<size_t>(1, batch * in_w)));
        HIP_TRY(sc.s_mmr_nf.ensure(batch * sizeof(uint32_t)));
        HIP_TRY(sc.s_rows.ensure(batch * out_w));
        HIP_TRY(sc.s_dist.ensure(batch * out_w));
        HIP_TRY(sc.s_out.ensure(batch * out_w));
        HIP_TRY(sc.s_nfound.ensure(batch * sizeof(uint32_t)));
        const MmrIo io{sc.s_mmr_rows.as<uint32_t>(), sc.s_mmr_dist.as<float>(), n_found_in ? sc.s_mmr_nf.as<uint32_t>() : nullptr,
                       sc.s_rows.as<uint32_t>(), sc.s_dist.as<float>(), sc.s_out.as<float>(), sc.s_nfound.as<uint32_t>()};
        for (uint32_t q0 = 0; q0 < nq; q0 += batch) {
            const uint32_t b = std::min<uint32_t>(batch, nq - q0);
            const size_t qi = static_cast<size_t>(q0) * n, qo = static_cast<size_t>(q0) * k;
            if (n) {
                HIP_TRY(hipMemcpyAsync(sc.s_mmr_rows.p, cand_rows + qi, b * in_w, hipMemcpyHostToDevice, rs->stream));
                HIP_TRY(hipMemcpyAsync(sc.s_mmr_dist.p, cand_dist + qi, b * in_w, hipMemcpyHostToDevice, rs->stream));
            }
            if (n_found_in) HIP_TRY(hipMemcpyAsync(sc.s_mmr_nf.p, n_found_in + q0, b * sizeof(uint32_t), hipMemcpyHostToDevice, rs->stream));
            if (int rc = enqueue_mmr(rs, map, io, b, n, k, lambda, mt, so, rs->stream)) return rc;
            HIP_TRY(hipMemcpyAsync(row_idx + qo, sc.s_rows.p, b * out_w, hipMemcpyDeviceToHost, rs->stream));
            HIP_TRY(hipMemcpyAsync(dist + qo, sc.s_dist.p, b * out_w, hipMemcpyDeviceToHost, rs->stream));
            if (score) HIP_TRY(hipMemcpyAsync(score + qo, sc.s_out.p, b * out_w, hipMemcpyDeviceToHost, rs->stream));
            if (n_found) HIP_TRY(hipMemcpyAsync(n_found + q0, sc.s_nfound.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost, rs->stream));
            HIP_TRY(hipStreamSynchronize(rs->stream));
            rs->counters.queries += b;
        }
        return lane.release();
    });
}
// Stage 1 into the lane, then the selection over it: for the queries d_queries [nq] of `s` (the searcher whose rows are read) on
// `stream`.  rq: a masked call's request, else nullptr; the picks go to io's outputs, stage 1's candidate totals to d_n_cand.
static int enqueue_topk_mmr(const pqv_searcher *s, Scratch &sc, const RowMap &map, const SearchRequest *rq, const float *d_queries, uint32_t nq,
                            uint32_t k, uint32_t fetch_k, float lambda, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out, MmrIo io,
                            uint64_t *d_n_cand, hipStream_t stream) {
    const size_t cells = static_cast<size_t>(nq) * fetch_k;
    HIP_TRY(sc.s_mmr_rows.ensure(cells * sizeof(uint32_t)));
    HIP_TRY(sc.s_mmr_dist.ensure(cells * sizeof(float)));
    HIP_TRY(sc.s_mmr_nf.ensure(static_cast<size_t>(nq) * sizeof(uint32_t)));
    if (int rc = enqueue_topk(s, d_queries, nq, fetch_k, fetch_k, nprobe, max_candidates, metric, sqrt_out, sc.s_mmr_rows.as<uint32_t>(),
                              sc.s_mmr_dist.as<float>(), sc.s_mmr_nf.as<uint32_t>(), d_n_cand, nullptr, stream, sc, rq))
        return rc;
    io.rows = sc.s_mmr_rows.as<uint32_t>(); io.dist = sc.s_mmr_dist.as<float>(); io.nf_in = sc.s_mmr_nf.as<uint32_t>();
    return enqueue_mmr(s, map, io, nq, fetch_k, k, lambda, metric, sqrt_out, stream);
}
// a masked call's request (mask NULL: none)
static const SearchRequest *mmr_request(const pqv_row_mask *mask, SearchRequest &mv) {
    if (!mask) return nullptr;
    mv = SearchRequest{};
    mv.rows.bits = mask->d_bits.as<uint64_t>(); mv.rows.mask = mask;
    return &mv;
}
extern "C" int pqv_topk_mmr_device(const pqv_searcher *s, const pqv_row_mask *mask, const void *d_queries, uint32_t nq, uint32_t k, uint32_t fetch_k,
                                   float lambda, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out, void *d_row_idx, void *d_dist,
                                   void *d_score, void *d_n_found, void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        if (int rc = mmr_checks(s, mask, k, fetch_k, lambda, true, nprobe, metric, false, 0)) return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!d_queries || !d_row_idx || !d_dist) return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        RowMap map{};
        if (int rc = ensure_row_map(s, map)) return rc;
        hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
        SearchRequest mv{};
        const SearchRequest *rq = mmr_request(mask, mv);
        const MmrIo io{nullptr, nullptr, nullptr, static_cast<uint32_t *>(d_row_idx), static_cast<float *>(d_dist), static_cast<float *>(d_score),
                       static_cast<uint32_t *>(d_n_found)};
        return partition_device_call(s, static_cast<const float *>(d_queries), nq, metric, sqrt_out ? 1 : 0, stream,
                                     [&](const pqv_searcher *bs, Scratch &sc, const float *q, int mt, int so) {
                                         return enqueue_topk_mmr(bs, sc, map, rq, q, nq, k, fetch_k, lambda, nprobe, max_candidates, mt, so, io,
                                                                 static_cast<uint64_t *>(d_n_candidates), stream);
                                     });
    });
}
extern "C" int pqv_topk_mmr(const pqv_searcher *s, const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                            uint32_t fetch_k, float lambda, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out, uint32_t *row_idx,
                            float *dist, float *score, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        if (int rc = mmr_checks(s, mask, k, fetch_k, lambda, true, nprobe, metric, true, query_len)) return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!queries || !row_idx || !dist) return fail(PQV_ERR_INVALID, "queries/row_idx/dist must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        RowMap map{};
        if (int rc = ensure_row_map(s, map)) return rc;
        SearchRequest mv{};
        const SearchRequest *rq = mmr_request(mask, mv);
        const pqv_searcher *bs = s;
        const float *qs = queries;
        int mt = metric, so = sqrt_out ? 1 : 0;
        std::vector<float> nq_host;
        if (int rc = cosine_queries_host(bs, qs, nq, mt, so, nq_host)) return rc;
        std::lock_guard<std::mutex> lock(bs->mu);
        Lane lane;
        if (int rc = lane.acquire(bs, bs->stream)) return rc;
        Scratch &sc = *lane;
        // the sub-batch bound of the plain host top-k at k = fetch_k, and stage 1's block and the picks beside it
        const TopkPlan p1 = plan_topk(bs, std::min<uint32_t>(nq, 1024), nprobe, fetch_k, mt, stream_request(rq));
        const uint64_t per_query = static_cast<uint64_t>(p1.n_part_rr) * fetch_k * 12 + static_cast<uint64_t>(p1.n_part_probe) * p1.probe_kpart * 12 +
                                   static_cast<uint64_t>(cand_cap_for(bs, fetch_k)) * 12 + static_cast<uint64_t>(p1.np) * (bs->sdim + 32) +
                                   static_cast<uint64_t>(bs->sdim) * 4 + 8ull * fetch_k + 12ull * k + 17;
        const uint32_t batch = static_cast<uint32_t>(std::max<uint64_t>(1, std::min<uint64_t>(nq, (1ull << 30) / per_query)));
        const size_t out_w = static_cast<size_t>(k) * sizeof(uint32_t);
        const std::vector<BatchOut> outs = {{&sc.s_rows, out_w, row_idx}, {&sc.s_dist, out_w, dist}, {&sc.s_out, out_w, score},
                                            {&sc.s_nfound, sizeof(uint32_t), n_found}, {&sc.s_ncand, sizeof(uint64_t), n_candidates}};
        if (int rc = host_batches(
                bs, sc, qs, nq, batch, rq, nullptr, outs,
                [&](uint32_t b, SearchRequest *brq) {
                    const MmrIo io{nullptr, nullptr, nullptr, sc.s_rows.as<uint32_t>(), sc.s_dist.as<float>(), sc.s_out.as<float>(), sc.s_nfound.as<uint32_t>()};
                    return enqueue_topk_mmr(bs, sc, map, brq, sc.s_queries.as<float>(), b, k, fetch_k, lambda, nprobe, max_candidates, mt, so, io,
                                            sc.s_ncand.as<uint64_t>(), bs->stream);
                },
                [](uint32_t, uint32_t) { return static_cast<int>(PQV_OK); }))      // (no host step: stage 1 replays nothing)
            return rc;
        return lane.release();
    });
}

// ---- range search over a key partition (pqv.h: pqv_range_search_partition) --------------------------------------------------------
// Per piece of PartitionWalk: the queries and the filter slice uploaded as the top-k host form uploads them, the walk stage's ONE
// span launch, and n_cand [b] brought back -- the one synchronisation this call has over range_body: the hit segments are
// PACKED, query q's holds n_cand[q] entries, and the grid follows the longest sequence.  The piece is then cut into groups of
// consecutive queries whose segments fit the byte budget (12 B an entry; partition_range_bytes, 0 = 1 GiB; a query whose own segment
// exceeds it runs alone).  Per group: hit_cnt zeroed, partition_range_kernel on the group's slice of the span arrays, the counts
// back, and range_body's write-out (range_write_out) over the packed segments.  A group without a candidate launches nothing.
// Timing: one event set per group that launches (the first of a piece begins ahead of the span launch); the range kernel is the
// "re-rank".
static int range_partition_body(const pqv_searcher *s, Scratch &sc, const pqv_key_partition *part, const pqv_key_filter *f, const uint64_t *bits,
                                const float *queries, uint32_t nq, float radius, uint64_t max_results, int metric, int sqrt_out, uint64_t *lims,
                                std::unique_ptr<uint32_t, HostFree> &rows, std::unique_ptr<float, HostFree> &dist, uint64_t *n_within,
                                uint64_t *n_candidates) {
    using namespace pqv;
    hipStream_t st = s->stream;
    const uint64_t budget = s->opt.partition_range_bytes ? s->opt.partition_range_bytes : (1ull << 30);
    PartitionWalk w{s, sc, part, f->kind, bits, metric, st};
    if (int rc = w.size(nq)) return rc;
    const uint32_t piece = w.piece, span_w = w.span_w();
    HIP_TRY(sc.s_queries.ensure(static_cast<size_t>(piece) * s->dim * sizeof(float)));
    HIP_TRY(sc.s_hit_cnt.ensure(static_cast<size_t>(piece) * sizeof(uint32_t)));
    HIP_TRY(sc.s_rout_off.ensure(static_cast<size_t>(piece) * sizeof(uint64_t)));
    HIP_TRY(sc.s_seg_off.ensure(static_cast<size_t>(piece) * sizeof(uint64_t)));
    const SearchRequest rq = partition_request(f);
    SearchRequest sub = rq;
    std::vector<uint64_t> sub_lims, h_ncand(piece), h_off(piece), h_seg(piece);
    std::vector<uint32_t> h_cnt(piece);
    std::vector<RangeSeg> segs;
    uint64_t cap_rows = 1, cap_dist = 1;      // entries the library buffers have room for
    for (uint32_t q0 = 0; q0 < nq; q0 += piece) {
        const uint32_t b = std::min<uint32_t>(piece, nq - q0);
        uint32_t launches = 0;
        hipEvent_t e[4];
        if (int rc = timing_events(s, e)) return rc;
        bool e_open = e[0] != nullptr;      // a set whose first event is recorded and whose others wait for a group
        HIP_TRY(hipMemcpyAsync(sc.s_queries.p, queries + static_cast<uint64_t>(q0) * s->dim, static_cast<size_t>(b) * s->dim * sizeof(float),
                               hipMemcpyHostToDevice, st));
        if (int rc = upload_query_filter(sc, &rq, sub, q0, b, sub_lims, st)) return rc;
        if (e[0]) HIP_TRY(hipEventRecord(e[0], st));
        StreamArgs pra;      // the piece's walk: every group runs on a slice of it
        PartitionArgs ppa;
        // (the piece's own filter slice: an IN filter's lims are rebased)
        if (int rc = w.launch(sc.s_queries.as<float>(), b, sub.d_filter_a(), sub.d_filter_b(), nullptr, pra, ppa)) return rc;
        launches += w.padded() ? 2 : 1;
        HIP_TRY(hipMemcpyAsync(h_ncand.data(), sc.s_ncand.p, static_cast<size_t>(b) * sizeof(uint64_t), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (n_candidates) std::copy(h_ncand.begin(), h_ncand.begin() + b, n_candidates + q0);

        for (uint32_t g0 = 0; g0 < b;) {
            // the group [g0, g1): consecutive queries while their segments fit the budget; never empty
            uint64_t entries = 0, longest = 0;
            uint32_t g1 = g0;
            while (g1 < b && (g1 == g0 || (entries + h_ncand[g1]) * 12 <= budget)) {
                h_seg[g1 - g0] = entries;
                entries += h_ncand[g1];
                longest = std::max(longest, h_ncand[g1]);
                ++g1;
            }
            const uint32_t gb = g1 - g0;
            if (entries == 0) {         // nobody has a candidate: nothing is launched
                for (uint32_t i = g0; i < g1; ++i) {
                    lims[q0 + i + 1] = lims[q0 + i];
                    if (n_within) n_within[q0 + i] = 0;
                }
                g0 = g1;
                continue;
            }
            if (!e_open) {
                if (int rc = timing_events(s, e)) return rc;
                if (e[0]) HIP_TRY(hipEventRecord(e[0], st));
            }
            e_open = false;
            HIP_TRY(sc.s_hit_keys.ensure(static_cast<size_t>(entries) * sizeof(uint64_t)));
            HIP_TRY(sc.s_hit_vals.ensure(static_cast<size_t>(entries) * sizeof(uint32_t)));
            HIP_TRY(hipMemsetAsync(sc.s_hit_cnt.p, 0, static_cast<size_t>(gb) * sizeof(uint32_t), st));
            HIP_TRY(hipMemcpyAsync(sc.s_seg_off.p, h_seg.data(), static_cast<size_t>(gb) * sizeof(uint64_t), hipMemcpyHostToDevice, st));
            // blocks per query: the option, or by rule about 2048 blocks for the group and no more than the longest sequence's turns
            uint64_t B = s->opt.partition_blocks;
            if (!B) B = std::min<uint64_t>((2048 + static_cast<uint64_t>(gb) - 1) / gb, (longest + 255) / 256);
            StreamArgs ra = pra;
            ra.queries = pra.queries + static_cast<size_t>(g0) * s->sdim; ra.nq = gb; ra.k = 1;
            ra.blocks_per_list = static_cast<uint32_t>(std::max<uint64_t>(1, B));
            ra.radius = radius; ra.sqrt_out = sqrt_out;
            ra.hit_cnt = sc.s_hit_cnt.as<uint32_t>(); ra.hit_keys = sc.s_hit_keys.as<uint64_t>(); ra.hit_vals = sc.s_hit_vals.as<uint32_t>();
            ra.seg_stride = 0; ra.seg_off = sc.s_seg_off.as<uint64_t>();
            PartitionArgs pa = ppa;
            // (the span arrays are indexed by the piece's query: IN keeps KEY_SET_MAX slots a query)
            pa.span_beg = ppa.span_beg + static_cast<size_t>(g0) * span_w;
            if (w.kind == PQV_KEY_IN) { pa.span_end = ppa.span_end + static_cast<size_t>(g0) * span_w; pa.n_span = ppa.n_span + g0; }
            pa.n_cand = ppa.n_cand + g0;
            if (e[1]) HIP_TRY(hipEventRecord(e[1], st));
            HIP_TRY(launch_partition_range(ra, pa, st));
            ++launches;
            if (e[2]) HIP_TRY(hipEventRecord(e[2], st));
            HIP_TRY(hipMemcpyAsync(h_cnt.data(), sc.s_hit_cnt.p, static_cast<size_t>(gb) * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            RangeWriteOut wo{sc.s_hit_cnt.as<uint32_t>(), h_cnt.data(), h_ncand.data() + g0, 0, sc.s_seg_off.as<uint64_t>(), max_results, metric, sqrt_out};
            if (int rc = range_write_out(s, sc, wo, q0 + g0, gb, lims, rows, dist, cap_rows, cap_dist, n_within, h_off, segs, e[3], launches)) return rc;
            g0 = g1;
        }
        if (e_open) for (int i = 1; i < 4; ++i) HIP_TRY(hipEventRecord(e[i], st));     // (a piece without a candidate)
        s->counters.queries += b;
        s->counters.kernel_launches += launches;
    }
    return PQV_OK;
}
// The family's checks (no k, no limit of its own), then pqv_range_search's own.
static int range_search_partition_impl(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *f, const pqv_row_mask *mask,
                                       const float *queries, uint32_t nq, uint32_t query_len, float radius, uint64_t max_results, int metric,
                                       int sqrt_out, uint64_t **lims_out, uint32_t **rows_out, float **dist_out, uint64_t *n_within,
                                       uint64_t *n_candidates) {
    if (int rc = partition_checks(s, part, f, nullptr, nullptr, mask, nq, 1, metric, true, query_len, nullptr)) return rc;
    if (metric == PQV_DOT) sqrt_out = 0;      // (ignored: the range_* kernels run as order-only machinery)
    if (std::isnan(radius)) return fail(PQV_ERR_INVALID, "radius must not be NaN");
    if (!lims_out || !rows_out || !dist_out) return fail(PQV_ERR_INVALID, "lims/row_idx/dist must not be NULL");
    if (nq && !queries) return fail(PQV_ERR_INVALID, "queries must not be NULL");
    *lims_out = nullptr; *rows_out = nullptr; *dist_out = nullptr;
    std::unique_ptr<uint64_t, HostFree> lims(static_cast<uint64_t *>(std::malloc((static_cast<size_t>(nq) + 1) * sizeof(uint64_t))));
    std::unique_ptr<uint32_t, HostFree> rows(static_cast<uint32_t *>(std::malloc(sizeof(uint32_t))));
    std::unique_ptr<float, HostFree> dist(static_cast<float *>(std::malloc(sizeof(float))));
    if (!lims || !rows || !dist) return fail(PQV_ERR_OOM, "host allocation failed");
    lims.get()[0] = 0;
    std::vector<float> nq_host;
    if (nq) {
        if (int rc = use_device(s->device)) return rc;
        // (PQV_COSINE: the L2 body on the cosine searcher over n(q): hits 0.5 d2 <= radius, written out halved)
        if (int rc = cosine_queries_host(s, queries, nq, metric, sqrt_out, nq_host)) return rc;
        const uint64_t *bits = mask ? mask->d_bits.as<uint64_t>() : nullptr;
        std::lock_guard<std::mutex> lock(s->mu);
        Lane lane;
        if (int rc = lane.acquire(s, s->stream)) return rc;
        if (int rc = range_partition_body(s, *lane, part, f, bits, queries, nq, radius, max_results, metric, sqrt_out, lims.get(), rows, dist,
                                          n_within, n_candidates))
            return rc;
        if (int rc = lane.release()) return rc;
    }
    *lims_out = lims.release(); *rows_out = rows.release(); *dist_out = dist.release();
    return PQV_OK;
}
extern "C" int pqv_range_search_partition(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *filter,
                                          const pqv_row_mask *mask, const float *queries, uint32_t nq, uint32_t query_len, float radius,
                                          uint64_t max_results, int metric, int sqrt_out, uint64_t **lims, uint32_t **row_idx, float **dist,
                                          uint64_t *n_within, uint64_t *n_candidates) {
    return guard([&] {
        return range_search_partition_impl(s, part, filter, mask, queries, nq, query_len, radius, max_results, metric, sqrt_out ? 1 : 0, lims,
                                           row_idx, dist, n_within, n_candidates);
    });
}

// ---- distinct / grouped top-k over a key partition (pqv.h: pqv_topk_partition_grouped) ------------------------------------------
// Enqueue both passes for the queries [0, nq) on `stream`, in PartitionWalk's pieces: the span kernel (once per piece), the
// distinct stream, and GroupFold's fold with the grouped stream over the same spans as its pass-2 walk.  One B for both passes;
// every buffer of a piece is sized before its first kernel.  `s`: the searcher whose rows are read; a / b: the descriptor's DEVICE
// arrays; out: the call's outputs.
static int enqueue_partition_grouped(const pqv_searcher *s, Scratch &sc, const pqv_key_partition *part, uint32_t kind, const void *d_a,
                                     const void *d_b, const pqv_row_keys *gk, const uint64_t *bits, const float *d_queries, uint32_t nq, uint32_t k,
                                     uint32_t m, int metric, int sqrt_out, const TopkOut &out, hipStream_t stream) {
    using namespace pqv;
    PartitionWalk w{s, sc, part, kind, bits, metric, stream};
    if (int rc = w.size(nq)) return rc;
    const uint32_t km = k * m;                                              // (<= 1024: partition_checks)
    const uint32_t B = partition_blocks(s, w.piece, km, part->m);
    const GroupFold fold{k, m, B * waves_per_block(), gk, sqrt_out};
    if (int rc = fold.size(sc, w.piece, out)) return rc;
    for (uint32_t q0 = 0; q0 < nq; q0 += w.piece) {
        const uint32_t b = std::min<uint32_t>(w.piece, nq - q0);
        const TopkOut o = fold.on_lane(sc, out.at(q0, k, km));
        StreamArgs ra;
        PartitionArgs pa;
        if (int rc = w.launch_at(q0, b, d_queries, d_a, d_b, o, ra, pa)) return rc;
        ra.k = k; ra.blocks_per_list = B;
        ra.part_keys = sc.s_part_keys.as<uint64_t>(); ra.part_vals = sc.s_part_vals.as<uint32_t>();
        DistinctArgs da{};
        da.key_pos = gk->d_key_pos.p; da.valid_pos = gk->valid_image(); da.elem_size = gk->elem_size();
        da.part_grp = sc.s_part_grp.as<int64_t>();
        HIP_TRY(launch_partition_distinct_stream(ra, pa, da, stream));
        s->counters.kernel_launches += 3;
        if (int rc = fold.enqueue(s, sc, stream, ra, o, [&](GroupedArgs &ga) {
                HIP_TRY(launch_partition_grouped_stream(ra, pa, ga, stream));
                return static_cast<int>(PQV_OK);
            }))
            return rc;
    }
    return PQV_OK;
}
extern "C" int pqv_topk_partition_grouped_device(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *filter,
                                                 const pqv_row_keys *group_keys, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                                 uint32_t k, uint32_t group_size, int metric, int sqrt_out, void *d_row_idx, void *d_dist,
                                                 void *d_group_key, void *d_group_rows, void *d_n_found, void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        if (int rc = partition_checks(s, part, filter, group_keys, &group_size, mask, nq, k, metric, false, 0,
                                      "pqv_topk_partition_grouped takes k * group_size <= 1024"))
            return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!d_queries || !d_row_idx || !d_dist) return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : s->stream;
        const uint64_t *bits = mask ? mask->d_bits.as<uint64_t>() : nullptr;
        const TopkOut out{static_cast<uint32_t *>(d_row_idx), static_cast<float *>(d_dist), static_cast<uint32_t *>(d_n_found),
                          static_cast<uint64_t *>(d_n_candidates), static_cast<int64_t *>(d_group_key), static_cast<uint32_t *>(d_group_rows)};
        return partition_device_call(s, static_cast<const float *>(d_queries), nq, metric, sqrt_out ? 1 : 0, stream,
                                     [&](const pqv_searcher *bs, Scratch &sc, const float *q, int mt, int so) {
                                         return enqueue_partition_grouped(bs, sc, part, filter->kind, filter->a, filter->b, group_keys, bits, q, nq, k,
                                                                          group_size, mt, so, out, stream);
                                     });
    });
}
extern "C" int pqv_topk_partition_grouped(const pqv_searcher *s, const pqv_key_partition *part, const pqv_key_filter *filter,
                                          const pqv_row_keys *group_keys, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                          uint32_t query_len, uint32_t k, uint32_t group_size, int metric, int sqrt_out, uint32_t *row_idx,
                                          float *dist, int64_t *group_key, uint32_t *group_rows, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        if (int rc = partition_checks(s, part, filter, group_keys, &group_size, mask, nq, k, metric, true, query_len,
                                      "pqv_topk_partition_grouped takes k * group_size <= 1024"))
            return rc;
        if (nq == 0) return static_cast<int>(PQV_OK);
        if (!queries || !row_idx || !dist) return fail(PQV_ERR_INVALID, "queries/row_idx/dist must not be NULL");
        if (int rc = use_device(s->device)) return rc;
        // (the scratch of BOTH passes: 20 B per entry of pass 1's lists, 16 B per entry of k * m and a count in pass 2's; the group
        // outputs beside the rows)
        const uint32_t m = group_size;
        const uint64_t km = static_cast<uint64_t>(k) * m;
        return topk_partition_host_body(
            s, part->m, partition_request(filter), mask, queries, nq, static_cast<uint32_t>(km), metric, sqrt_out ? 1 : 0,
            std::max<uint64_t>(std::max<uint64_t>(k * 20ull, km * 12), m > 1 ? km * 16 + 4 : 0), 32ull * k + 8 * km + 8 * PQV_KEY_SET_MAX + 16,
            PartitionHostOuts{{row_idx, dist, n_found, n_candidates, group_key, group_rows}, k, km, true},
            [&](const pqv_searcher *bs, Scratch &sc, const uint64_t *bits, const void *d_a, const void *d_b, uint32_t b, int mt, int so,
                const TopkOut &out) {
                return enqueue_partition_grouped(bs, sc, part, filter->kind, d_a, d_b, group_keys, bits, sc.s_queries.as<float>(), b, k, m, mt, so,
                                                 out, bs->stream);
            });
    });
}

// ---- distinct top-k (pqv.h: pqv_topk_distinct) -----------------------------------------------------------------------------
// the checks both entry points make before anything else: NULL handles first, nothing dereferenced before them
static int distinct_view(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_row_mask *mask, uint32_t k, SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!keys) return fail(PQV_ERR_INVALID, "row keys must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");       // (validate_topk's, ahead of everything that reads a handle)
    if (keys->owner != s || keys->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "row keys belong to another searcher");
    mv = SearchRequest{};
    if (mask) {
        if (int rc = mask_view(s, mask, mv)) return rc;
    }
    mv.groups.col = keys;
    return PQV_OK;
}
namespace {
// Beyond the kernels' lists (k > 1024 or more than 1024 probed lists): the (d2, position)-sorted considered rows of every query from
// the masked range machinery -- radius +inf, d2 out, under the position image (key validity AND shared mask) -- and the first row
// of every key value kept on the host.  Correct for any k / nprobe; not a fast path.
// m (a grouped call, pqv.h: pqv_topk_grouped): the first m rows of each of those key values, row_idx / dist [nq, k, m], group_rows [nq, k].
int distinct_unbounded(const pqv_searcher *s, Scratch &sc, const SearchRequest *mv, const float *queries, uint32_t nq, uint32_t k, uint32_t nprobe,
                       uint64_t max_candidates, int metric, int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key,
                       uint32_t *n_found, uint64_t *n_candidates, uint32_t m, uint32_t *group_rows) {
    const pqv_row_keys *gk = mv->groups.col;
    if (int rc = keys_host_rows(s, gk)) return rc;
    // the image of the considered positions, made on the host from the two images (n / 8 bytes each)
    const uint64_t n_words = (s->n + 63) / 64 + 1;
    std::vector<uint64_t> img, other;
    try { img.assign(n_words, ~0ull); other.resize(n_words); } catch (const std::bad_alloc &) { return fail(PQV_ERR_OOM, "host allocation failed"); }
    for (const void *src : {gk->has_valid ? gk->d_valid_pos.p : nullptr, static_cast<void *>(const_cast<uint64_t *>(mv->rows.bits))}) {
        if (!src) continue;
        HIP_TRY(hipMemcpy(other.data(), src, n_words * sizeof(uint64_t), hipMemcpyDeviceToHost));
        for (uint64_t w = 0; w < n_words; ++w) img[w] &= other[w];
    }
    for (uint64_t pz = s->n; pz < n_words * 64; ++pz) img[pz >> 6] &= ~(1ull << (pz & 63u));     // (bits of positions >= n are zero)
    DevBuf d_img;
    HIP_TRY(d_img.alloc(n_words * sizeof(uint64_t)));
    HIP_TRY(hipMemcpy(d_img.p, img.data(), n_words * sizeof(uint64_t), hipMemcpyHostToDevice));
    SearchRequest rv{};
    rv.rows.bits = d_img.as<uint64_t>();
    // (a filtered call: the per-query filter travels beside the image, as in pqv_range_search_filtered)
    rv.rows.keys = mv->rows.keys; rv.rows.h_qkeys = mv->rows.h_qkeys; rv.rows.kind = mv->rows.kind; rv.rows.h_a = mv->rows.h_a; rv.rows.h_b = mv->rows.h_b;
    std::unique_ptr<uint64_t, HostFree> lims(static_cast<uint64_t *>(std::malloc((static_cast<size_t>(nq) + 1) * sizeof(uint64_t))));
    std::unique_ptr<uint32_t, HostFree> rows(static_cast<uint32_t *>(std::malloc(sizeof(uint32_t))));
    std::unique_ptr<float, HostFree> d2(static_cast<float *>(std::malloc(sizeof(float))));
    if (!lims || !rows || !d2) return fail(PQV_ERR_OOM, "host allocation failed");
    lims.get()[0] = 0;
    if (int rc = range_body(s, sc, queries, nq, INFINITY, nprobe, max_candidates, 0, metric, 0, lims.get(), rows, d2, nullptr, n_candidates, &rv))
        return rc;
    std::unordered_map<int64_t, uint32_t> slot_of;       // key value -> its group's rank
    std::vector<uint32_t> have;                          // rows kept per group
    for (uint32_t q = 0; q < nq; ++q) {
        slot_of.clear();
        have.clear();
        uint32_t found = 0;
        uint64_t open = 0;                               // groups that still take rows
        const uint64_t qo = static_cast<uint64_t>(q) * k;
        uint32_t *orow = row_idx + qo * m;
        float *od = dist + qo * m;
        int64_t *og = group_key ? group_key + qo : nullptr;
        uint32_t *ogr = group_rows ? group_rows + qo : nullptr;
        for (uint64_t i = lims.get()[q]; i < lims.get()[q + 1] && (found < k || open); ++i) {
            const uint32_t r = rows.get()[i];
            if (r >= gk->n_rows) continue;
            const int64_t g = gk->host_vals[r];
            uint32_t slot;
            const auto it = slot_of.find(g);
            if (it != slot_of.end()) {
                slot = it->second;
                if (have[slot] >= m) continue;
            } else {
                if (found >= k) continue;
                slot = found++;
                slot_of.emplace(g, slot);
                have.push_back(0);
                if (og) og[slot] = g;
                ++open;
            }
            const float v = d2.get()[i];
            const uint64_t o = static_cast<uint64_t>(slot) * m + have[slot];
            orow[o] = r;
            od[o] = sqrt_out == 1 ? std::sqrt(v) : sqrt_out == 2 ? 0.5f * v : v;
            if (++have[slot] == m) --open;
        }
        // (k may be huge -- "keep everything": the caller's buffers are [nq * k * m] all the same)
        for (uint64_t e = 0; e < k; ++e) {
            const uint32_t h = e < found ? have[e] : 0u;
            for (uint64_t i = h; i < m; ++i) { orow[e * m + i] = 0xFFFFFFFFu; od[e * m + i] = INFINITY; }
            if (og && e >= found) og[e] = 0;
            if (ogr) ogr[e] = h;
        }
        if (n_found) n_found[q] = found;
    }
    return PQV_OK;
}
}  // namespace
extern "C" int pqv_topk_distinct(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                 uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                 uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = distinct_view(s, keys, mask, k, mv)) return rc;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates,
                             &mv, group_key);
    });
}
extern "C" int pqv_topk_distinct_device(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_row_mask *mask, const void *d_queries,
                                        uint32_t nq, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                        void *d_row_idx, void *d_dist, void *d_group_key, void *d_n_found, void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = distinct_view(s, keys, mask, k, mv)) return rc;
        mv.groups.d_keys = static_cast<int64_t *>(d_group_key);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, nullptr, hip_stream, &mv);
    });
}

// ---- grouped top-k (pqv.h: pqv_topk_grouped) ---------------------------------------------------------------------------------
// distinct_view's checks with "group_size must be > 0" behind "k must be > 0" (both ahead of everything that reads a handle)
static int grouped_view(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_row_mask *mask, uint32_t k, uint32_t group_size, SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!keys) return fail(PQV_ERR_INVALID, "row keys must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (group_size == 0) return fail(PQV_ERR_INVALID, "group_size must be > 0");
    if (int rc = distinct_view(s, keys, mask, k, mv)) return rc;
    mv.groups.size = group_size;
    return PQV_OK;
}
extern "C" int pqv_topk_grouped(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                uint32_t query_len, uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates, int metric,
                                int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows, uint32_t *n_found,
                                uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = grouped_view(s, keys, mask, k, group_size, mv)) return rc;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates,
                             &mv, group_key, group_rows);
    });
}
extern "C" int pqv_topk_grouped_device(const pqv_searcher *s, const pqv_row_keys *keys, const pqv_row_mask *mask, const void *d_queries,
                                       uint32_t nq, uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates, int metric,
                                       int sqrt_out, void *d_row_idx, void *d_dist, void *d_group_key, void *d_group_rows, void *d_n_found,
                                       void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = grouped_view(s, keys, mask, k, group_size, mv)) return rc;
        mv.groups.d_keys = static_cast<int64_t *>(d_group_key);
        mv.groups.d_rows = static_cast<uint32_t *>(d_group_rows);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, nullptr, hip_stream, &mv);
    });
}

// ---- distinct / grouped top-k under a per-query key filter (pqv.h: pqv_topk_distinct_filtered) ---------------------------------
// Both halves of the view in the contract's order: every NULL and zero check, the descriptor's included, before a handle is read.
// group_size: nullptr for the distinct forms.
static int group_filtered_view(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys, const pqv_key_filter *filter,
                               const pqv_row_mask *mask, uint32_t nq, uint32_t k, const uint32_t *group_size, bool host, SearchRequest &mv) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!group_keys) return fail(PQV_ERR_INVALID, "row keys must not be NULL");
    if (!filter_keys) return fail(PQV_ERR_INVALID, "a key filter needs row keys");
    if (!filter) return fail(PQV_ERR_INVALID, "filter must not be NULL");
    if (int rc = filter_descriptor_checks(filter, nq, host)) return rc;
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (group_size && *group_size == 0) return fail(PQV_ERR_INVALID, "group_size must be > 0");
    if (group_keys->owner != s || group_keys->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "row keys belong to another searcher");
    // (the filter column's owner and the mask's: filtered_view)
    if (int rc = filtered_view(s, filter_keys, filter, nq, mask, host, mv, true)) return rc;
    mv.groups.col = group_keys;
    mv.groups.size = group_size ? *group_size : 0u;
    return PQV_OK;
}
extern "C" int pqv_topk_distinct_filtered(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                          const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                          uint32_t query_len, uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                          uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *n_found, uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_filtered_view(s, group_keys, filter_keys, filter, mask, nq, k, nullptr, true, mv)) return rc;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates,
                             &mv, group_key);
    });
}
extern "C" int pqv_topk_distinct_filtered_device(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                                 const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                                 uint32_t k, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out, void *d_row_idx,
                                                 void *d_dist, void *d_group_key, void *d_n_found, void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_filtered_view(s, group_keys, filter_keys, filter, mask, nq, k, nullptr, false, mv)) return rc;
        mv.groups.d_keys = static_cast<int64_t *>(d_group_key);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, nullptr, hip_stream, &mv);
    });
}
extern "C" int pqv_topk_grouped_filtered(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                         const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                         uint32_t query_len, uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates, int metric,
                                         int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows, uint32_t *n_found,
                                         uint64_t *n_candidates) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_filtered_view(s, group_keys, filter_keys, filter, mask, nq, k, &group_size, true, mv)) return rc;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates,
                             &mv, group_key, group_rows);
    });
}
extern "C" int pqv_topk_grouped_filtered_device(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                                const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                                uint32_t k, uint32_t group_size, uint32_t nprobe, uint64_t max_candidates, int metric, int sqrt_out,
                                                void *d_row_idx, void *d_dist, void *d_group_key, void *d_group_rows, void *d_n_found,
                                                void *d_n_candidates, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_filtered_view(s, group_keys, filter_keys, filter, mask, nq, k, &group_size, false, mv)) return rc;
        mv.groups.d_keys = static_cast<int64_t *>(d_group_key);
        mv.groups.d_rows = static_cast<uint32_t *>(d_group_rows);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, max_candidates, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found,
                                    d_n_candidates, nullptr, hip_stream, &mv);
    });
}

// ---- expanding distinct / grouped top-k (pqv.h: pqv_topk_distinct_expand) ------------------------------------------------------
// The checks of all four forms up to the view, in the contract's order: every NULL and zero check before a handle is read.
// group_size: nullptr for the distinct forms.
static int group_expand_view(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys, const pqv_key_filter *filter,
                             const pqv_row_mask *mask, uint32_t nq, uint32_t k, const uint32_t *group_size, uint32_t nprobe, uint32_t max_nprobe,
                             int metric, bool host, SearchRequest &mv) {
    const char *name = group_size ? "pqv_topk_grouped_expand" : "pqv_topk_distinct_expand";
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (!group_keys) return fail(PQV_ERR_INVALID, "row keys must not be NULL");
    if (!filter_keys && filter) return fail(PQV_ERR_INVALID, "a key filter needs row keys");
    if (filter_keys && !filter) return fail(PQV_ERR_INVALID, "filter must not be NULL");
    if (filter_keys) { if (int rc = filter_descriptor_checks(filter, nq, host)) return rc; }
    if (max_nprobe < nprobe) return fail(PQV_ERR_INVALID, "max_nprobe must be >= nprobe");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (group_size && *group_size == 0) return fail(PQV_ERR_INVALID, "group_size must be > 0");
    if (group_keys->owner != s || group_keys->owner_uid != s->uid) return fail(PQV_ERR_INVALID, "row keys belong to another searcher");
    if (filter_keys) {      // (the filter column's owner and the mask's: filtered_view)
        if (int rc = filtered_view(s, filter_keys, filter, nq, mask, host, mv, true)) return rc;
    } else {
        mv = SearchRequest{};
        if (mask) { if (int rc = mask_view(s, mask, mv)) return rc; }
    }
    mv.groups.col = group_keys;
    mv.groups.size = group_size ? *group_size : 0u;
    if (int rc = validate_topk(s, k, nprobe, metric)) return rc;
    if (s->n_files) return fail(PQV_ERR_UNSUPPORTED, std::string(name) + " does not take table searchers");
    if (int rc = dot_checks(s, 1, 1, metric, &mv)) return rc;
    if (static_cast<uint64_t>(k) * std::max<uint32_t>(1, mv.groups.size) > 1024 || probe_count(s, max_nprobe) > 1024)
        return fail(PQV_ERR_UNSUPPORTED, std::string(name) + (group_size ? " takes k * group_size <= 1024" : " takes k <= 1024") +
                                             " and at most 1024 probed lists per query");
    mv.expand.max_nprobe = max_nprobe;
    return PQV_OK;
}
extern "C" int pqv_topk_distinct_expand(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                        const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                        uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t max_nprobe, int metric, int sqrt_out,
                                        uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *n_found, uint64_t *n_candidates,
                                        uint32_t *nprobe_used) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_expand_view(s, group_keys, filter_keys, filter, mask, nq, k, nullptr, nprobe, max_nprobe, metric, true, mv)) return rc;
        mv.expand.h_used = nprobe_used;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, 0, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates,
                             &mv, group_key);
    });
}
extern "C" int pqv_topk_distinct_expand_device(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                               const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                               uint32_t k, uint32_t nprobe, uint32_t max_nprobe, int metric, int sqrt_out, void *d_row_idx,
                                               void *d_dist, void *d_group_key, void *d_n_found, void *d_n_candidates, void *d_nprobe_used,
                                               void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_expand_view(s, group_keys, filter_keys, filter, mask, nq, k, nullptr, nprobe, max_nprobe, metric, false, mv)) return rc;
        mv.groups.d_keys = static_cast<int64_t *>(d_group_key);
        mv.expand.d_used = static_cast<uint32_t *>(d_nprobe_used);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, 0, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found, d_n_candidates,
                                    nullptr, hip_stream, &mv);
    });
}
extern "C" int pqv_topk_grouped_expand(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                       const pqv_key_filter *filter, const pqv_row_mask *mask, const float *queries, uint32_t nq,
                                       uint32_t query_len, uint32_t k, uint32_t group_size, uint32_t nprobe, uint32_t max_nprobe, int metric,
                                       int sqrt_out, uint32_t *row_idx, float *dist, int64_t *group_key, uint32_t *group_rows, uint32_t *n_found,
                                       uint64_t *n_candidates, uint32_t *nprobe_used) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_expand_view(s, group_keys, filter_keys, filter, mask, nq, k, &group_size, nprobe, max_nprobe, metric, true, mv)) return rc;
        mv.expand.h_used = nprobe_used;
        return pqv_topk_impl(s, queries, nq, query_len, k, nprobe, 0, metric, sqrt_out ? 1 : 0, row_idx, dist, n_found, n_candidates,
                             &mv, group_key, group_rows);
    });
}
extern "C" int pqv_topk_grouped_expand_device(const pqv_searcher *s, const pqv_row_keys *group_keys, const pqv_row_keys *filter_keys,
                                              const pqv_key_filter *filter, const pqv_row_mask *mask, const void *d_queries, uint32_t nq,
                                              uint32_t k, uint32_t group_size, uint32_t nprobe, uint32_t max_nprobe, int metric, int sqrt_out,
                                              void *d_row_idx, void *d_dist, void *d_group_key, void *d_group_rows, void *d_n_found,
                                              void *d_n_candidates, void *d_nprobe_used, void *hip_stream) {
    return guard([&] {
        SearchRequest mv{};
        if (int rc = group_expand_view(s, group_keys, filter_keys, filter, mask, nq, k, &group_size, nprobe, max_nprobe, metric, false, mv)) return rc;
        mv.groups.d_keys = static_cast<int64_t *>(d_group_key);
        mv.groups.d_rows = static_cast<uint32_t *>(d_group_rows);
        mv.expand.d_used = static_cast<uint32_t *>(d_nprobe_used);
        return pqv_topk_device_impl(s, d_queries, nq, k, nprobe, 0, metric, sqrt_out ? 1 : 0, d_row_idx, d_dist, d_n_found, d_n_candidates,
                                    nullptr, hip_stream, &mv);
    });
}

static int pqv_searcher_set_option_impl(pqv_searcher *s, const char *name, int64_t value) {
    if (!s || !name) return fail(PQV_ERR_INVALID, "searcher/name must not be NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    pqv_searcher::Opts &o = s->opt;
    const std::string n(name);
    if (n == "rerank_mode") o.rerank_mode = static_cast<int>(value);
    else if (n == "tile_filter") o.tile_filter = static_cast<int>(std::min<int64_t>(2, std::max<int64_t>(0, value)));
    else if (n == "filter_variant") o.filter_variant = static_cast<int>(value);
    else if (n == "cand_cap") o.cand_cap = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "screen_f16") o.screen_f16 = value != 0;
    else if (n == "screen_i8") o.screen_i8 = static_cast<int>(value);
    else if (n == "seed_rows") o.seed_rows = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "wide_rows") o.wide_rows = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "tile_rows") o.tile_rows = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "running_thr") o.running_thr = value != 0;
    else if (n == "defer") o.defer = static_cast<int>(value);
    else if (n == "quad_xcd") o.quad_xcd = static_cast<int>(value);
    else if (n == "wide_waves") o.wide_waves = static_cast<int>(value);
    else if (n == "single_bucket") o.single_bucket = static_cast<int>(value);      // 2 = bucketing in the merge, separate probe launch
    else if (n == "seed_refine") o.seed_refine = static_cast<int>(value);       // 2 = any dim / batch size
    else if (n == "item_grid") o.item_grid = static_cast<int>(value);          // 2 = also for the 8-wave blocks
    else if (n == "chunk_major") o.chunk_major = value != 0;
    else if (n == "probe_rows") o.probe_rows = static_cast<int>(value);       // 2 = for any batch size
    else if (n == "probe_screen") {       // 0 = off, 2 = every batch the kernels support
        o.probe_screen = static_cast<int>(value);
        // a searcher created with the option off (PQV_PROBE_SCREEN=0) has no images yet: made here, once
        if (value != 0 && !s->ps.tried && s->kc_pad != 0 && !s->n_files) {
            const hipError_t e = probe_screen_images(s);
            if (e != hipSuccess) return fail(e == hipErrorOutOfMemory ? PQV_ERR_OOM : PQV_ERR_HIP, std::string("probe_screen_images: ") + hipGetErrorString(e));
        }
    }
    else if (n == "quad_width") o.quad_width = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "min_blocks") o.min_blocks = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "pair_prune") o.pair_prune = value != 0;
    else if (n == "wide_quads") o.wide_quads = value <= 0 ? 0 : value >= 2 ? 2 : 1;       // 1: by the previous batch's shape; 2: always
    else if (n == "fork_wide") o.fork_wide = value <= 0 ? 0 : value >= 2 ? 2 : 1;
    else if (n == "pf96") o.pf96 = value <= 0 ? 0 : value >= 2 ? 2 : 1;
    else if (n == "static_dim") o.static_dim = value != 0 ? 1 : 0;
    else if (n == "drain_min") o.drain_min = static_cast<int>(std::max<int64_t>(0, std::min<int64_t>(64, value)));
    else if (n == "xcd_items") o.xcd_items = static_cast<int>(std::max<int64_t>(0, std::min<int64_t>(3, value)));
    else if (n == "wide_quad_rows") o.wide_quad_rows = static_cast<uint32_t>(std::max<int64_t>(0, value));
    else if (n == "list_once") o.list_once = static_cast<int>(value);
    else if (n == "partition_blocks") o.partition_blocks = static_cast<uint32_t>(std::max<int64_t>(0, std::min<int64_t>(4096, value)));
    else if (n == "partition_range_bytes") o.partition_range_bytes = static_cast<uint64_t>(std::max<int64_t>(0, value));
    else if (n == "i8_form") {        // takes effect when the int8 copy is (re)built
        o.i8_form = static_cast<int>(std::min<int64_t>(2, std::max<int64_t>(0, value)));
        (void)hipSetDevice(s->device);
        (void)hipDeviceSynchronize();          // nothing in flight may still read the copy
        s->d_mat_blk_op[2].release();
    }
    else return fail(PQV_ERR_INVALID, "unknown searcher option: " + n);
    if (s->cos) return pqv_searcher_set_option_impl(s->cos.get(), name, value);      // (the cosine searcher follows)
    return PQV_OK;
}
extern "C" int pqv_searcher_set_option(pqv_searcher *s, const char *name, int64_t value) {
    return guard([&] { return pqv_searcher_set_option_impl(s, name, value); });
}

static int pqv_searcher_describe_impl(const pqv_searcher *s, uint32_t nq, uint32_t k, uint32_t nprobe, int metric,
                                      char *buf, size_t len) {
    if (!s || !buf || !len) return fail(PQV_ERR_INVALID, "searcher/buf must not be NULL");
    if (int rc = validate_topk(s, k, nprobe, metric)) return rc;
    if (int rc = dot_checks(s, k, nprobe, metric, nullptr)) return rc;
    if (metric == PQV_COSINE) {
        // the L2 dispatch of the cosine searcher (before the first cosine call: of this one, over the raw rows)
        const pqv_searcher *c;
        {
            std::lock_guard<std::mutex> lock(s->mu);
            c = s->cos ? s->cos.get() : s;
        }
        const int l = std::snprintf(buf, len, "PQV_COSINE%s: normalize_rows_kernel (n(q), one launch on the call's stream), then ",
                                    c == s ? " (layout not built yet)" : "");
        const size_t used = l < 0 ? 0 : std::min<size_t>(static_cast<size_t>(l), len - 1);
        if (int rc = pqv_searcher_describe_impl(c, nq, k, nprobe, PQV_L2SQ_REF4, buf + used, len - used)) return rc;
        const size_t end = std::strlen(buf);
        std::snprintf(buf + end, len - end, "; distances halved in the final write-out (merge_kernel / range write-out)");
        return PQV_OK;
    }
    std::lock_guard<std::mutex> lock(s->mu);
    // a table names itself first: its files, the lists a query probes, and the probe route
    char tb[256] = "";
    if (s->n_files) {
        const TopkPlan pt = plan_topk(s, std::max<uint32_t>(1, nq), nprobe, k, metric);
        std::snprintf(tb, sizeof tb, "table of %u files, %u lists per query (nprobe %u per file); probe: %s + merge_probe_seg_kernel (per file), "
                      "no fused single-query probe (pair sort instead); ", s->n_files, probe_count(s, nprobe), nprobe,
                      beyond_kernel_lists(s, k, nprobe) ? "stream_kernel (STREAM_DIST) + a stable sort per file on the host"
                      : pt.probe_rows ? "probe_rows_kernel" : metric == PQV_DOT ? "dot_stream_kernel with one list per file" : "stream_kernel with one list per file");
    }
    if (beyond_kernel_lists(s, k, nprobe)) {
        std::snprintf(buf, len, "%spqv_topk only: stream_kernel (STREAM_DIST) for every centroid and candidate distance, selection by the "
                                "reference's heap on the host (k > 1024 or min(nprobe, n_clusters) > 1024)", tb);
        return PQV_OK;
    }
    const TopkPlan p = plan_topk(s, std::max<uint32_t>(1, nq), nprobe, k, metric);
    const TopkRoute rt = topk_route(s, p, std::max<uint32_t>(1, nq), k);      // the decisions enqueue_topk follows
    char t[1024];
    if (rt.screened)
        std::snprintf(t, sizeof t, "wide_seed_kernel + seed_select_kernel + wide_filter_kernel: %s screen operands, quads of %u queries "
                      "staged %s, %u waves per block, %u rows per block, threshold sample %u rows per list%s%s",
                      rt.operand == 2 ? "int8" : rt.operand == 1 ? "f16" : "f32", p.quad_width,
                      !rt.q_global ? "in LDS" : "as a blocked copy in global memory",
                      p.block_waves, p.filter_rows_per_block, p.seed_rows,
                      seed_refine_on(s, std::max<uint32_t>(1, nq), k) ? " + exact refinement" : "",
                      !p.i8 ? "" : !s->d_mat_blk_op[2].p ? "" : s->i8_residual ? "; int8 images of the per-list residual (one per probed pair)" : "; int8 images about one centre (one per query)");
    else if (p.tile && p.filter)
        std::snprintf(t, sizeof t, "tile_rerank_kernel (exact seed window of %u rows) + tile_filter_kernel: 16-query groups, f32 screen operands, "
                      "%u rows per block", p.seed_rows, p.filter_rows_per_block);
    else if (p.tile)
        std::snprintf(t, sizeof t, "tile_rerank_kernel: exact arithmetic, 16-query groups, %u rows per block", p.rr_rows_per_block);
    else if (metric == PQV_DOT)
        std::snprintf(t, sizeof t, "PQV_DOT: dot_stream_kernel (a masked call: its WIN = 1 form over the mask's set positions): one candidate "
                      "stream per (query, probed list), %u rows per block, keys (ord(dist) << 32) | position; dot_merge_kernel (range search: "
                      "range_* sort kernels + dot_finish_kernel)", p.rr_rows_per_block);
    else
        std::snprintf(t, sizeof t, "stream_kernel: one candidate stream per (query, probed list), %u rows per block", p.rr_rows_per_block);
    if (rt.screened && p.wide_width) {
        const size_t l = std::strlen(t);
        if (p.list_once)
            std::snprintf(t + l, sizeof t - l, "; lists probed by more than %u queries: list_filter_kernel -- 32 rows per wave stationary in registers, all the list's pairs "
                          "(quads of up to %u) streamed past them in chunks of 32: every such list read once, %u rows per block", p.quad_width, p.wide_width, p.wide_rows_per_block);
        else
        std::snprintf(t + l, sizeof t - l, "; lists probed by %u..%u queries: one quad, 8 waves per block on 32-row tiles, %u rows per block",
                      p.quad_width + 1, p.wide_width, p.wide_rows_per_block);
    }
    if (rt.screened && rt.operand == 2) {
        // (launch_wide's rule: the regular and the wide-quad int8 instance, k <= 64, exact evaluation in the kernel, 768 dims)
        const bool sd = s->opt.static_dim && s->sdim == 768 && k <= 64 && !rt.deferred && !rt.q_global && p.quad_width == 96 && p.block_waves == 4;
        const size_t l = std::strlen(t);
        if (sd) std::snprintf(t + l, sizeof t - l, "; row length compiled in (%u dims: unrolled K loops, A operands at four lane addresses + immediates)", s->sdim);
        else std::snprintf(t + l, sizeof t - l, "; row length read at run time");
    }
    if (rt.deferred) {
        const size_t l = std::strlen(t);
        std::snprintf(t + l, sizeof t - l, "; exact evaluations deferred: survivors appended with their bounds, resolve_select_kernel + "
                                           "resolve_exact_kernel evaluate what the k-th smallest upper bound leaves");
    }
    if (s->sdim != s->dim) {
        const size_t l = std::strlen(t);
        std::snprintf(t + l, sizeof t - l, "; rows stored zero-padded from %u to %u dims", s->dim, s->sdim);
    }
    // exact instantiations (as rocprofv3 prints them), so that a profile line can be matched to this dispatch
    char kn[384] = "";
    if (rt.screened) {
        const int S = k <= 64 ? 1 : 4;
        const bool qlds = !rt.q_global;
        const bool pf = p.f16 && s->sdim <= 128 && p.block_waves == 4 && p.quad_width != 96;
        const int op = rt.operand;
        const int seed_ng = p.i8 ? (64ull * s->sdim <= 49152 ? 4 : 2) : p.f16 ? ((64ull * s->sdim * 2 <= 32768 && p.quad_width % 64 == 0) ? 4 : 2) : static_cast<int>(p.quad_width / 16);
        const bool defp = S == 1 && rt.deferred;
        std::snprintf(kn, sizeof kn, " | kernels: wide_filter_kernel<%u, %u, %d, %s, %d, %s, %s, 4, %s>; wide_seed_kernel<%d, %s, %d, %d>; seed_select_kernel<%d>@%u",
                      p.quad_width / 16, p.block_waves, S, qlds ? "true" : "false", op, pf ? "true" : "false",
                      ((p.i8 && p.block_waves == 4 && p.quad_width == 64 && std::max<uint32_t>(1, nq) <= 64u) || p.wide_width) ? "true" : "false",
                      defp ? "true" : "false", seed_ng, qlds ? "true" : "false", op, rt.seed_tail ? 12 : 1, S,
                      std::max<uint32_t>(1, nq) * (seed_refine_on(s, std::max<uint32_t>(1, nq), k) ? 256u : 64u));
        if (p.wide_width) {
            const size_t l = std::strlen(kn);
            if (p.list_once) std::snprintf(kn + l, sizeof kn - l, "; list_filter_kernel<%u, %d>", s->sdim / 64, S);
            else
            std::snprintf(kn + l, sizeof kn - l, "; wide_filter_kernel<%u, 8, %d, true, 2, false, %s, 2, %s>", p.wide_width / 16, S, wide_rows_nt(s) ? "true" : "false",
                          defp ? "true" : "false");
        }
    }
    if (metric == PQV_DOT) {
        const bool al = (s->sdim % 4) == 0;
        std::snprintf(kn, sizeof kn, " | kernels: dot_stream_kernel<%d, %d, 0, %s, 0>; dot_merge_kernel<%d>",
                      (al && (s->sdim / 4) % 64 == 0) ? 64 : 32, k <= 64 ? 1 : k <= 256 ? 4 : 16, al ? "true" : "false", k <= 64 ? 1 : k <= 256 ? 4 : 16);
    }
    std::snprintf(buf, len, "%s%s; centroid probe: %s%s", tb, t, p.probe_screen ? "probe_screen_kernel + probe_resolve_kernel (f16 contraction, probe_rows_kernel's exact chains for the contenders)"
                  : p.probe_rows ? "probe_rows_kernel (a lane per centroid)" : metric == PQV_DOT ? "dot_stream_kernel" : "stream_kernel", kn);
    return PQV_OK;
}
extern "C" int pqv_searcher_describe(const pqv_searcher *s, uint32_t nq, uint32_t k, uint32_t nprobe, int metric,
                                     char *buf, size_t len) {
    return guard([&] { return pqv_searcher_describe_impl(s, nq, k, nprobe, metric, buf, len); });
}

static int pqv_searcher_footprint_impl(const pqv_searcher *s, uint64_t *row_order_bytes, uint64_t *ivf_rows_bytes,
                                       uint64_t *blocked_bytes, uint64_t *other_bytes) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    if (row_order_bytes) *row_order_bytes = s->corpus && s->corpus->d_rows ? s->corpus->capacity * s->corpus->dim * sizeof(float) : 0;
    if (ivf_rows_bytes) *ivf_rows_bytes = s->d_mat_ivf.p ? s->d_mat_ivf.bytes : 0;
    if (blocked_bytes) *blocked_bytes = (s->d_mat_blk_op[0].p ? s->d_mat_blk_op[0].bytes : 0) + (s->d_mat_blk_op[1].p ? s->d_mat_blk_op[1].bytes : 0) +
                                        (s->d_mat_blk_op[2].p ? s->d_mat_blk_op[2].bytes : 0);
    uint64_t other = s->d_centroids.bytes + s->d_cent_t.bytes + s->d_ps_mu.bytes + s->d_ps_c16.bytes + s->d_ps_cn2.bytes + s->d_ps_stats.bytes + s->d_list_off.bytes + s->d_ids.bytes + s->d_row_map.bytes + s->d_stats.bytes + s->d_row_norm2.bytes + s->d_blk_off.bytes +
                     s->d_center.bytes + s->d_list_scale.bytes + s->d_list_half.bytes + s->d_list_radius.bytes + s->d_row_n2i.bytes + s->d_row_res.bytes;
    for (const Scratch &l : s->lanes)
        for (const DevBuf *b : l.bufs()) other += b->p ? b->bytes : 0;
    if (other_bytes) *other_bytes = other;
    if (s->cos) {       // the cosine layout: its searcher's buffers, its normalised row-order copy included, in the same four classes
        uint64_t f[4] = {0, 0, 0, 0};
        if (int rc = pqv_searcher_footprint_impl(s->cos.get(), f, f + 1, f + 2, f + 3)) return rc;
        if (row_order_bytes) *row_order_bytes += f[0];
        if (ivf_rows_bytes) *ivf_rows_bytes += f[1];
        if (blocked_bytes) *blocked_bytes += f[2];
        if (other_bytes) *other_bytes += f[3];
    }
    return PQV_OK;
}
extern "C" int pqv_searcher_footprint(const pqv_searcher *s, uint64_t *row_order_bytes, uint64_t *ivf_rows_bytes,
                                      uint64_t *blocked_bytes, uint64_t *other_bytes) {
    return guard([&] { return pqv_searcher_footprint_impl(s, row_order_bytes, ivf_rows_bytes, blocked_bytes, other_bytes); });
}

static int pqv_probe_impl(const pqv_searcher *s, const float *query, uint32_t query_len, uint32_t nprobe,
                         uint32_t *clusters_out, uint32_t *n_out) {
    if (int rc = validate_query(s, 1, nprobe, PQV_L2SQ_REF4, 0, query_len)) return rc;
    if (!query || !clusters_out) return fail(PQV_ERR_INVALID, "query/clusters_out must not be NULL");
    const uint32_t np = probe_count(s, nprobe);
    if (int rc = use_device(s->device)) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    Lane lane;
    if (int rc = lane.acquire(s, s->stream)) return rc;
    Scratch &sc = *lane;
    HIP_TRY(sc.s_queries.ensure(static_cast<size_t>(s->dim) * sizeof(float)));
    HIP_TRY(hipMemcpyAsync(sc.s_queries.p, query, static_cast<size_t>(s->dim) * sizeof(float), hipMemcpyHostToDevice, s->stream));
    if (np > 1024) {            // beyond the kernels' sorted lists: distances on the GPU, the stable sort on the host
        std::vector<uint32_t> clusters;
        uint64_t total = 0;
        if (int rc = host_probe(s, sc, sc.s_queries.as<float>(), 1, nprobe, 0, false, clusters, &total)) return rc;
        std::memcpy(clusters_out, clusters.data(), static_cast<size_t>(np) * sizeof(uint32_t));
        if (n_out) *n_out = np;
        return lane.release();
    }
    const TopkPlan p = plan_topk(s, 1, nprobe);
    pqv::MergeArgs pm{};        // (no pm.stats: a probe counts no candidates)
    if (int rc = probe_merge_args(s, sc, p, 1, 0, pm)) return rc;
    if (int rc = enqueue_probe(s, sc, p, sc.s_queries.as<float>(), 1, nprobe, 0, pm, nullptr, 0, s->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(clusters_out, sc.s_probe.p, static_cast<size_t>(np) * sizeof(uint32_t),
                           hipMemcpyDeviceToHost, s->stream));
    if (int rc = lane.release()) return rc;
    HIP_TRY(hipStreamSynchronize(s->stream));
    if (n_out) *n_out = np;
    s->counters.kernel_launches += 2;
    return PQV_OK;
}
extern "C" int pqv_probe(const pqv_searcher *s, const float *query, uint32_t query_len, uint32_t nprobe,
                         uint32_t *clusters_out, uint32_t *n_out) {
    return guard([&] { return pqv_probe_impl(s, query, query_len, nprobe, clusters_out, n_out); });
}

static int pqv_candidate_rows_impl(const pqv_searcher *s, const float *query, uint32_t query_len,
                                  uint32_t nprobe, uint32_t **rows, uint64_t *n_rows) {
    if (!rows || !n_rows) return fail(PQV_ERR_INVALID, "rows/n_rows must not be NULL");
    *rows = nullptr; *n_rows = 0;
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    const uint32_t np = probe_count(s, nprobe);
    std::vector<uint32_t> clusters(std::max<uint32_t>(np, 1));
    uint32_t got = 0;
    if (int rc = pqv_probe(s, query, query_len, nprobe, clusters.data(), &got)) return rc;
    uint64_t total = 0;
    for (uint32_t i = 0; i < got; ++i) total += s->h_list_off[clusters[i] + 1] - s->h_list_off[clusters[i]];
    const std::vector<uint32_t> *h_rows = s->h_rows->get();             // (downloaded by the first call that reads them)
    if (!h_rows) return PQV_ERR_HIP;
    uint32_t *buf = static_cast<uint32_t *>(std::malloc(std::max<uint64_t>(1, total) * sizeof(uint32_t)));
    if (!buf) return fail(PQV_ERR_OOM, "host allocation failed");
    uint64_t o = 0;
    for (uint32_t i = 0; i < got; ++i) {  // probe-rank major, ascending ids inside (index.rs:59-62)
        const uint64_t b = s->h_list_off[clusters[i]], e = s->h_list_off[clusters[i] + 1];
        std::memcpy(buf + o, h_rows->data() + b, (e - b) * sizeof(uint32_t));
        o += e - b;
    }
    *rows = buf; *n_rows = total;
    s->counters.candidate_rows += total;
    return PQV_OK;
}
extern "C" int pqv_candidate_rows(const pqv_searcher *s, const float *query, uint32_t query_len,
                                  uint32_t nprobe, uint32_t **rows, uint64_t *n_rows) {
    return guard([&] { return pqv_candidate_rows_impl(s, query, query_len, nprobe, rows, n_rows); });
}

extern "C" void pqv_rows_free(uint32_t *rows) { std::free(rows); }

static int pqv_counters_impl(const pqv_searcher *s, pqv_counters_t *out) {
    if (!s || !out) return fail(PQV_ERR_INVALID, "searcher/out must not be NULL");
    if (int rc = use_device(s->device)) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    unsigned long long st[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIP_TRY(hipMemcpy(st, s->d_stats.p, sizeof st, hipMemcpyDeviceToHost));   // synchronises the device
#ifndef PQV_PROFILE_PHASES
    {   // wide_filter_kernel spreads its two counters over STATS_SLOTS lines
        std::vector<unsigned long long> slots(16 * pqv::STATS_SLOTS);
        HIP_TRY(hipMemcpy(slots.data(), static_cast<const unsigned long long *>(s->d_stats.p) + 8,
                          slots.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        for (uint32_t i = 0; i < pqv::STATS_SLOTS; ++i) {
            st[0] += slots[16 * i]; st[1] += slots[16 * i + 1]; st[2] += slots[16 * i + 2]; st[3] += slots[16 * i + 3];
        }
    }
#endif
#ifdef PQV_PROFILE_PHASES
    {
        std::vector<unsigned long long> rec(8 + 8 * 65536);
        HIP_TRY(hipMemcpy(rec.data(), s->d_stats.p, rec.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost));
        if (const char *path = std::getenv("PQV_PHASES_OUT")) {
            if (FILE *f = std::fopen(path, "wb")) { std::fwrite(rec.data(), sizeof(unsigned long long), rec.size(), f); std::fclose(f); }
        }
    }
#endif
    *out = s->counters;
    out->screened_pairs = st[0];
    out->screen_survivors = st[1];
    out->candidate_rows += st[2];         // top-k calls (device counters) + pqv_candidate_rows (host counter)
    out->embeddings_fetched += st[3];
    if (s->cos) {                         // PQV_COSINE calls count on the cosine searcher
        pqv_counters_t c{};
        if (int rc = pqv_counters_impl(s->cos.get(), &c)) return rc;
        out->queries += c.queries; out->candidate_rows += c.candidate_rows; out->embeddings_fetched += c.embeddings_fetched;
        out->kernel_launches += c.kernel_launches; out->exact_replays += c.exact_replays; out->screened_pairs += c.screened_pairs;
        out->screen_survivors += c.screen_survivors;
    }
    return PQV_OK;
}
extern "C" int pqv_counters(const pqv_searcher *s, pqv_counters_t *out) {
    return guard([&] { return pqv_counters_impl(s, out); });
}

static int pqv_set_timing_impl(pqv_searcher *s, int enabled) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    std::lock_guard<std::mutex> lock(s->mu);
    s->timing = enabled != 0;
    if (s->cos) return pqv_set_timing_impl(s->cos.get(), enabled);
    return PQV_OK;
}
extern "C" int pqv_set_timing(pqv_searcher *s, int enabled) {
    return guard([&] { return pqv_set_timing_impl(s, enabled); });
}

static int pqv_timing_read_impl(const pqv_searcher *s, double *rerank_ms, double *total_ms,
                               uint32_t *n_calls) {
    if (!s) return fail(PQV_ERR_INVALID, "searcher must not be NULL");
    if (int rc = use_device(s->device)) return rc;
    std::lock_guard<std::mutex> lock(s->mu);
    double rr = 0.0, tot = 0.0;
    uint32_t calls = 0;
    for (size_t i = 0; i + 3 < s->ev.size(); i += 4) {
        HIP_TRY(hipEventSynchronize(s->ev[i + 3]));
        float a = 0.f, b = 0.f;
        HIP_TRY(hipEventElapsedTime(&a, s->ev[i + 1], s->ev[i + 2]));
        HIP_TRY(hipEventElapsedTime(&b, s->ev[i], s->ev[i + 3]));
        rr += a; tot += b; calls++;
    }
    for (auto e : s->ev) (void)hipEventDestroy(e);
    s->ev.clear();
    if (s->cos) {                         // PQV_COSINE calls record on the cosine searcher
        double r2 = 0.0, t2 = 0.0;
        uint32_t c2 = 0;
        if (int rc = pqv_timing_read_impl(s->cos.get(), &r2, &t2, &c2)) return rc;
        rr += r2; tot += t2; calls += c2;
    }
    if (rerank_ms) *rerank_ms = rr;
    if (total_ms) *total_ms = tot;
    if (n_calls) *n_calls = calls;
    return PQV_OK;
}
extern "C" int pqv_timing_read(const pqv_searcher *s, double *rerank_ms, double *total_ms,
                               uint32_t *n_calls) {
    return guard([&] { return pqv_timing_read_impl(s, rerank_ms, total_ms, n_calls); });
}

// ---------------------------------------------------------------------------------------
// batched brute force on the matrix cores (BASELINE config 5; extension, see pqv.h)
// ---------------------------------------------------------------------------------------
static int pqv_brute_topk_impl(const pqv_corpus *c, const float *queries, uint32_t nq, uint32_t query_len,
                              uint32_t k, int metric, uint32_t *row_idx, float *dist, uint32_t *n_found) {
    using namespace pqv;
    if (!c) return fail(PQV_ERR_INVALID, "corpus must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (k > 1024) return fail(PQV_ERR_UNSUPPORTED, "k > 1024 is not supported");
    if (metric != PQV_COSINE && metric != PQV_L2SQ_MFMA)
        return fail(PQV_ERR_INVALID, "pqv_brute_topk: metric must be PQV_COSINE or PQV_L2SQ_MFMA");
    if (query_len != c->dim)
        return fail(PQV_ERR_INVALID, "Query dimension mismatch: expected " + std::to_string(c->dim) +
                                         ", got " + std::to_string(query_len));
    if (nq == 0) return PQV_OK;
    if (!queries || !row_idx || !dist) return fail(PQV_ERR_INVALID, "queries/row_idx/dist must not be NULL");
    if (!c->d_rows) return fail(PQV_ERR_INVALID, "corpus row-order copy was released");
    if (int rc = use_device(c->device)) return rc;
    hipStream_t stream = c->stream;
    const uint64_t n = c->n;
    const uint32_t dim = c->dim;
    const int mode = metric == PQV_COSINE ? 0 : 1;

    // per-row auxiliary (cached in the corpus, recomputed if rows were appended since)
    const float *d_row_aux = nullptr;
    {
        std::lock_guard<std::mutex> lock(c->aux_mu);
        DevBuf &buf = mode == 0 ? c->aux_rnorm : c->aux_norm2;
        uint64_t &have = mode == 0 ? c->aux_rnorm_rows : c->aux_norm2_rows;
        if (have != n || !buf.p) {
            HIP_TRY(buf.alloc(std::max<uint64_t>(1, n) * sizeof(float)));
            HIP_TRY(launch_row_norms(c->d_rows, n, dim, mode, buf.as<float>(), stream));
            HIP_TRY(hipStreamSynchronize(stream));
            have = n;
        }
        d_row_aux = buf.as<float>();
    }
    // Round 3: beyond the first row range the contraction runs on the f16 matrix pipe as a screen (kernels_brute.hip:
    // brute_f16_kernel) and only what it lets through is scored in f32.  Needs the normalised f16 image of the
    // corpus (+ 1 / |v| whatever the metric); PQV_BRUTE_F16=0 keeps the f32 contraction everywhere.
    // The screen's operand form: int8 images (twice the matrix rate, half the staged bytes; PQV_BRUTE_OP=f16 keeps the f16 images).
    static const bool f16_env = [] { const char *e = std::getenv("PQV_BRUTE_F16"); return !(e && *e == '0'); }();
    const bool i8_env = [] { const char *e = std::getenv("PQV_BRUTE_OP"); return !(e && !std::strcmp(e, "f16")); }();      // (read per call: tests run both forms)
    const bool use_i8 = i8_env;
    const uint32_t dim_p = use_i8 ? (dim + 63) / 64 * 64 : (dim + 31) / 32 * 32;
    const bool use_f16 = f16_env && n >= 32768 && static_cast<uint64_t>(dim_p) * 2 * 320 < 0x7FFFFFFFull;
    const uint16_t *d_v16 = nullptr;
    const int8_t *d_v8 = nullptr;
    const float4 *d_v8_sr = nullptr;
    const float *d_v8_n = nullptr;
    const float *d_vn2 = nullptr;
    if (use_f16 && use_i8) {
        std::lock_guard<std::mutex> lock(c->aux_mu);
        if (c->aux_rnorm_rows != n || !c->aux_rnorm.p) {
            HIP_TRY(c->aux_rnorm.alloc(std::max<uint64_t>(1, n) * sizeof(float)));
            HIP_TRY(launch_row_norms(c->d_rows, n, dim, 0, c->aux_rnorm.as<float>(), stream));
            c->aux_rnorm_rows = n;
        }
        if (mode == 1) d_vn2 = d_row_aux;
        if (c->aux_v8_rows != n || !c->aux_v8.p) {
            HIP_TRY(c->aux_v8.alloc(std::max<uint64_t>(1, n) * dim_p));
            HIP_TRY(c->aux_v8_sr.alloc(std::max<uint64_t>(1, n) * sizeof(float4)));
            HIP_TRY(c->aux_v8_n.alloc(std::max<uint64_t>(1, n) * sizeof(float)));
            HIP_TRY(c->aux_v8_max.alloc(12 * sizeof(float)));
            HIP_TRY(hipMemsetAsync(c->aux_v8_max.p, 0, 12 * sizeof(float), stream));
            HIP_TRY(launch_normalize_i8(c->d_rows, c->aux_rnorm.as<float>(), n, dim, dim_p, c->aux_v8.p, c->aux_v8_sr.p, c->aux_v8_n.as<float>(),
                                        c->aux_v8_max.as<float>(), stream));
            HIP_TRY(hipStreamSynchronize(stream));
            c->aux_v8_rows = n;
        }
        d_v8 = c->aux_v8.as<int8_t>(); d_v8_sr = c->aux_v8_sr.as<float4>(); d_v8_n = c->aux_v8_n.as<float>();
    } else if (use_f16) {
        std::lock_guard<std::mutex> lock(c->aux_mu);
        if (c->aux_rnorm_rows != n || !c->aux_rnorm.p) {
            HIP_TRY(c->aux_rnorm.alloc(std::max<uint64_t>(1, n) * sizeof(float)));
            HIP_TRY(launch_row_norms(c->d_rows, n, dim, 0, c->aux_rnorm.as<float>(), stream));
            c->aux_rnorm_rows = n;
        }
        if (mode == 1) d_vn2 = d_row_aux;
        if (c->aux_v16_rows != n || !c->aux_v16.p) {
            HIP_TRY(c->aux_v16.alloc(std::max<uint64_t>(1, n) * dim_p * sizeof(uint16_t)));
            HIP_TRY(launch_normalize_f16(c->d_rows, c->aux_rnorm.as<float>(), n, dim, dim_p, c->aux_v16.p, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            c->aux_v16_rows = n;
        }
        d_v16 = c->aux_v16.as<uint16_t>();
    }
    // (int8: the image bound is per pair, inside the kernel; eps carries the f32 roundings of the normalisation and of both sums)
    const float f16_eps = use_i8 ? 2.0f * static_cast<float>(dim_p) * 5.9604645e-08f + 4.0e-6f
                                 : 1.01f * 9.765625e-04f + 2.0f * static_cast<float>(dim_p) * 5.9604645e-08f + 2.0e-6f;

    const uint32_t cap = std::max<uint32_t>(16384, 4 * k);
    const uint32_t qbatch = std::min<uint32_t>(nq, 4096);
    DevBuf d_q, d_qaux, d_cand, d_cnt, d_cnt_saved, d_thr, d_flag, d_rows_out, d_dist_out, d_nf;
    HIP_TRY(d_q.alloc(static_cast<size_t>(qbatch) * dim * sizeof(float)));
    HIP_TRY(d_qaux.alloc(static_cast<size_t>(qbatch) * sizeof(float)));
    HIP_TRY(d_cand.alloc(static_cast<size_t>(qbatch) * cap * sizeof(unsigned long long)));
    HIP_TRY(d_cnt.alloc(static_cast<size_t>(qbatch) * sizeof(uint32_t)));
    HIP_TRY(d_cnt_saved.alloc(static_cast<size_t>(qbatch) * sizeof(uint32_t)));
    HIP_TRY(d_thr.alloc(static_cast<size_t>(qbatch) * sizeof(unsigned long long)));
    HIP_TRY(d_flag.alloc(sizeof(uint32_t)));
    HIP_TRY(d_rows_out.alloc(static_cast<size_t>(qbatch) * k * sizeof(uint32_t)));
    HIP_TRY(d_dist_out.alloc(static_cast<size_t>(qbatch) * k * sizeof(float)));
    HIP_TRY(d_nf.alloc(static_cast<size_t>(qbatch) * sizeof(uint32_t)));
    DevBuf d_q16, d_qrn, d_qsr, d_qn;
    if (use_f16) {
        HIP_TRY(d_q16.alloc(static_cast<size_t>(qbatch) * dim_p * sizeof(uint16_t)));
        HIP_TRY(d_qrn.alloc(static_cast<size_t>(qbatch) * sizeof(float)));
        if (use_i8) { HIP_TRY(d_qsr.alloc(static_cast<size_t>(qbatch) * sizeof(float4))); HIP_TRY(d_qn.alloc(static_cast<size_t>(qbatch) * sizeof(float))); }
    }

    for (uint32_t q0 = 0; q0 < nq; q0 += qbatch) {
        const uint32_t b = std::min<uint32_t>(qbatch, nq - q0);
        HIP_TRY(hipMemcpyAsync(d_q.p, queries + static_cast<uint64_t>(q0) * dim, static_cast<size_t>(b) * dim * sizeof(float),
                               hipMemcpyHostToDevice, stream));
        HIP_TRY(launch_row_norms(d_q.as<float>(), b, dim, mode, d_qaux.as<float>(), stream));
        if (use_f16) {
            HIP_TRY(launch_row_norms(d_q.as<float>(), b, dim, 0, d_qrn.as<float>(), stream));
            if (use_i8) HIP_TRY(launch_normalize_i8(d_q.as<float>(), d_qrn.as<float>(), b, dim, dim_p, d_q16.p, d_qsr.p, d_qn.as<float>(), nullptr, stream));
            else HIP_TRY(launch_normalize_f16(d_q.as<float>(), d_qrn.as<float>(), b, dim, dim_p, d_q16.p, stream));
        }
        HIP_TRY(hipMemsetAsync(d_cnt.p, 0, static_cast<size_t>(b) * sizeof(uint32_t), stream));
        HIP_TRY(hipMemsetAsync(d_thr.p, 0xFF, static_cast<size_t>(b) * sizeof(unsigned long long), stream));
        HIP_TRY(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), stream));

        // Progressive thresholds: row ranges grow 8x; after each range the per-query k-th key
        // becomes the admission threshold of the next, so only ~8k candidates per query
        // survive each pass.  A range whose survivors overflow a buffer (adversarially ordered
        // rows) is rolled back and split.
        std::vector<std::pair<uint64_t, uint64_t>> todo;
        {
            std::vector<std::pair<uint64_t, uint64_t>> fwd;
            // (the first range has no threshold yet, so EVERY pair of it is appended -- one atomic each: 8192 rows cost 3.8 ms on
            //  C5, a tenth of the step; 2048 rows seed thresholds that the next range tightens anyway)
            uint64_t lo = 0, len = std::min<uint64_t>(n, std::max<uint64_t>(use_f16 ? 2048 : 8192, 8ull * k));
            while (lo < n) {
                const uint64_t hi = std::min<uint64_t>(n, lo + len);
                fwd.emplace_back(lo, hi);
                lo = hi;
                len *= 8;
            }
            todo.assign(fwd.rbegin(), fwd.rend());   // stack: pop_back() yields ascending ranges
        }
        bool first_range = true;
        while (!todo.empty()) {
            const auto range = todo.back();
            todo.pop_back();
            HIP_TRY(hipMemcpyAsync(d_cnt_saved.p, d_cnt.p, static_cast<size_t>(b) * sizeof(uint32_t),
                                   hipMemcpyDeviceToDevice, stream));
            BruteArgs ba{};
            ba.rows = c->d_rows; ba.queries = d_q.as<float>(); ba.row_aux = d_row_aux; ba.query_aux = d_qaux.as<float>();
            ba.row_begin = range.first; ba.row_end = range.second; ba.nq = b; ba.dim = dim;
            ba.metric = mode == 0 ? BRUTE_COSINE : BRUTE_L2SQ;
            ba.thr = d_thr.as<unsigned long long>(); ba.cand = d_cand.as<unsigned long long>();
            ba.cand_cnt = d_cnt.as<uint32_t>(); ba.cap = cap;
            // the first range seeds the thresholds exactly; every later one is screened on the f16 pipe
            const bool screen = use_f16 && range.first > 0;
            if (screen) {
                BruteF16Args fa{};
                fa.v16 = d_v16; fa.q16 = d_q16.as<uint16_t>(); fa.row_aux = d_vn2; fa.query_aux = d_qaux.as<float>();
                if (use_i8) {
                    fa.v8 = d_v8; fa.q8 = d_q16.as<int8_t>(); fa.row_sr = d_v8_sr; fa.query_sr = d_qsr.as<float4>();
                    fa.row_n = d_v8_n; fa.query_n = d_qn.as<float>(); fa.dim_f = static_cast<float>(dim); fa.row_max = c->aux_v8_max.as<float>();
                    // a wave sums dim / 64 components per lane + 6 exchange steps: error <= (dim / 64 + 7) 2^-24 sum |v^_i| <= .. sqrt(dim)
                    fa.eps_sum = (static_cast<float>(dim) / 64.0f + 8.0f) * 5.9604645e-08f * std::sqrt(static_cast<float>(dim)) * 1.01f;
                }
                fa.row_begin = range.first; fa.row_end = range.second; fa.nq = b; fa.dim_p = dim_p;
                fa.metric = ba.metric; fa.eps = f16_eps;
                fa.thr = ba.thr; fa.cand = ba.cand; fa.cand_cnt = ba.cand_cnt; fa.cap = cap;
                HIP_TRY(launch_brute_f16(fa, stream));
            } else {
                // the very first range: nothing to compare with yet, every pair is kept -- written to its own slot instead of one
                // atomic append per pair (2048 rows x 1024 queries: 1.07 -> 0.1 ms on C5)
                const bool dense = first_range && range.second - range.first <= cap;
                ba.dense = dense ? 1u : 0u;
                HIP_TRY(launch_brute_mfma(ba, stream));
                if (dense) HIP_TRY(hipMemsetD32Async(static_cast<hipDeviceptr_t>(d_cnt.p), static_cast<int>(range.second - range.first), b, stream));
            }
            first_range = false;
            // overflow is checked BEFORE the select pass touches the buffer fronts, so a
            // rollback only has to restore the counts
            HIP_TRY(launch_brute_overflow_check(d_cnt.as<uint32_t>(), b, cap, d_flag.as<uint32_t>(), stream));
            uint32_t flag = 0;
            HIP_TRY(hipMemcpyAsync(&flag, d_flag.p, sizeof flag, hipMemcpyDeviceToHost, stream));
            HIP_TRY(hipStreamSynchronize(stream));
            if (flag) {
                const uint64_t len = range.second - range.first;
                if (len <= cap / 2)
                    return fail(PQV_ERR_HIP, "pqv_brute_topk: candidate buffer overflow on a minimal range");
                HIP_TRY(hipMemcpyAsync(d_cnt.p, d_cnt_saved.p, static_cast<size_t>(b) * sizeof(uint32_t),
                                       hipMemcpyDeviceToDevice, stream));
                HIP_TRY(hipMemsetAsync(d_flag.p, 0, sizeof(uint32_t), stream));
                const uint64_t mid = range.first + len / 2;
                todo.emplace_back(mid, range.second);
                todo.emplace_back(range.first, mid);
                continue;
            }
            if (screen && std::getenv("PQV_BRUTE_STATS")) {        // diagnostic: pairs the screen let through in this range
                std::vector<uint32_t> h1(b), h0(b);
                HIP_TRY(hipMemcpy(h1.data(), d_cnt.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost));
                HIP_TRY(hipMemcpy(h0.data(), d_cnt_saved.p, b * sizeof(uint32_t), hipMemcpyDeviceToHost));
                uint64_t t = 0;
                for (uint32_t i = 0; i < b; ++i) t += h1[i] - h0[i];
                std::fprintf(stderr, "pqv_brute_topk: rows [%llu, %llu): %.1f screen survivors per query\n",
                             (unsigned long long)range.first, (unsigned long long)range.second, (double)t / b);
            }
            if (screen) HIP_TRY(launch_brute_rescore(ba, d_cnt_saved.as<uint32_t>(), stream));     // exact f32 keys for what the screen let through
            HIP_TRY(launch_brute_select(d_cand.as<unsigned long long>(), d_cnt.as<uint32_t>(), cap, b, k,
                                        d_thr.as<unsigned long long>(), d_flag.as<uint32_t>(), stream));
        }
        HIP_TRY(launch_brute_finish(d_cand.as<unsigned long long>(), d_cnt.as<uint32_t>(), cap, b, k,
                                    d_rows_out.as<uint32_t>(), d_dist_out.as<float>(), d_nf.as<uint32_t>(), stream));
        HIP_TRY(hipMemcpyAsync(row_idx + static_cast<uint64_t>(q0) * k, d_rows_out.p, static_cast<size_t>(b) * k * sizeof(uint32_t),
                               hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipMemcpyAsync(dist + static_cast<uint64_t>(q0) * k, d_dist_out.p, static_cast<size_t>(b) * k * sizeof(float),
                               hipMemcpyDeviceToHost, stream));
        if (n_found)
            HIP_TRY(hipMemcpyAsync(n_found + q0, d_nf.p, static_cast<size_t>(b) * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
        HIP_TRY(hipStreamSynchronize(stream));
    }
    return PQV_OK;
}
extern "C" int pqv_brute_topk(const pqv_corpus *c, const float *queries, uint32_t nq, uint32_t query_len,
                              uint32_t k, int metric, uint32_t *row_idx, float *dist, uint32_t *n_found) {
    return guard([&] { return pqv_brute_topk_impl(c, queries, nq, query_len, k, metric, row_idx, dist, n_found); });
}

// ---------------------------------------------------------------------------------------
// host-side merge of per-shard lists (multi-file / multi-GPU)
// ---------------------------------------------------------------------------------------
static int pqv_merge_topk_impl(const float *dist, const uint32_t *rows, const uint32_t *counts,
                              uint32_t n_lists, uint32_t nq, uint32_t k, float *out_dist,
                              uint32_t *out_rows, uint32_t *out_list, uint32_t *out_count) {
    if (!dist || !rows || !counts || !out_dist || !out_rows)
        return fail(PQV_ERR_INVALID, "merge arrays must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    struct Item { float d; uint32_t list, pos, row; };
    std::vector<Item> items;
    for (uint32_t q = 0; q < nq; ++q) {
        items.clear();
        for (uint32_t l = 0; l < n_lists; ++l) {
            const uint32_t cnt = std::min<uint32_t>(counts[static_cast<uint64_t>(l) * nq + q], k);
            const uint64_t base = (static_cast<uint64_t>(l) * nq + q) * k;
            for (uint32_t i = 0; i < cnt; ++i) items.push_back({dist[base + i], l, i, rows[base + i]});
        }
        std::stable_sort(items.begin(), items.end(), [](const Item &a, const Item &b) {
            if (a.d < b.d) return true;
            if (b.d < a.d) return false;
            if (a.list != b.list) return a.list < b.list;
            return a.pos < b.pos;
        });
        const uint32_t take = static_cast<uint32_t>(std::min<size_t>(k, items.size()));
        for (uint32_t i = 0; i < k; ++i) {
            const uint64_t o = static_cast<uint64_t>(q) * k + i;
            if (i < take) {
                out_dist[o] = items[i].d; out_rows[o] = items[i].row;
                if (out_list) out_list[o] = items[i].list;
            } else {
                out_dist[o] = INFINITY; out_rows[o] = 0xFFFFFFFFu;
                if (out_list) out_list[o] = 0xFFFFFFFFu;
            }
        }
        if (out_count) out_count[q] = take;
    }
    return PQV_OK;
}
extern "C" int pqv_merge_topk(const float *dist, const uint32_t *rows, const uint32_t *counts,
                              uint32_t n_lists, uint32_t nq, uint32_t k, float *out_dist,
                              uint32_t *out_rows, uint32_t *out_list, uint32_t *out_count) {
    return guard([&] { return pqv_merge_topk_impl(dist, rows, counts, n_lists, nq, k, out_dist, out_rows, out_list, out_count); });
}

static int pqv_merge_topk_device_impl(int device, const void *d_dist, const void *d_rows, const void *d_row_base,
                                      uint32_t n_lists, uint32_t nq, uint32_t k, void *d_out_dist,
                                      void *d_out_rows, void *hip_stream) {
    if (!d_dist || !d_rows || !d_row_base || !d_out_dist || !d_out_rows)
        return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (k > 1024) return fail(PQV_ERR_UNSUPPORTED, "k > 1024 is not supported");
    if (n_lists == 0 || nq == 0) return PQV_OK;
    if (int rc = use_device(device)) return rc;
    HIP_TRY(pqv::launch_shard_merge(static_cast<const float *>(d_dist), static_cast<const uint32_t *>(d_rows),
                                    static_cast<const long long *>(d_row_base), n_lists, nq, k,
                                    static_cast<float *>(d_out_dist), static_cast<long long *>(d_out_rows),
                                    static_cast<hipStream_t>(hip_stream)));
    return PQV_OK;
}
extern "C" int pqv_merge_topk_device(int device, const void *d_dist, const void *d_rows, const void *d_row_base,
                                     uint32_t n_lists, uint32_t nq, uint32_t k, void *d_out_dist,
                                     void *d_out_rows, void *hip_stream) {
    return guard([&] { return pqv_merge_topk_device_impl(device, d_dist, d_rows, d_row_base, n_lists, nq, k,
                                                         d_out_dist, d_out_rows, hip_stream); });
}

static int pqv_merge_topk_packed_device_impl(int device, const void *d_pairs, const void *d_row_base, uint32_t n_lists,
                                             uint32_t nq, uint32_t k, void *d_out_dist, void *d_out_rows, void *hip_stream) {
    if (!d_pairs || !d_row_base || !d_out_dist || !d_out_rows)
        return fail(PQV_ERR_INVALID, "device pointers must not be NULL");
    if (k == 0) return fail(PQV_ERR_INVALID, "k must be > 0");
    if (k > 1024) return fail(PQV_ERR_UNSUPPORTED, "k > 1024 is not supported");
    if (n_lists == 0 || nq == 0) return PQV_OK;
    if (int rc = use_device(device)) return rc;
    const float *base = static_cast<const float *>(d_pairs);
    HIP_TRY(pqv::launch_shard_merge(base, reinterpret_cast<const uint32_t *>(base) + 1,
                                    static_cast<const long long *>(d_row_base), n_lists, nq, k,
                                    static_cast<float *>(d_out_dist), static_cast<long long *>(d_out_rows),
                                    static_cast<hipStream_t>(hip_stream), 2));
    return PQV_OK;
}
extern "C" int pqv_merge_topk_packed_device(int device, const void *d_pairs, const void *d_row_base, uint32_t n_lists,
                                            uint32_t nq, uint32_t k, void *d_out_dist, void *d_out_rows, void *hip_stream) {
    return guard([&] { return pqv_merge_topk_packed_device_impl(device, d_pairs, d_row_base, n_lists, nq, k, d_out_dist,
                                                                d_out_rows, hip_stream); });
}

// ---------------------------------------------------------------------------------------
// CandidateCursor (src/df_vector/access.rs:193-243)
// ---------------------------------------------------------------------------------------
struct pqv_candidate_cursor {
    std::vector<std::vector<uint32_t>> candidates;
    std::vector<uint64_t> positions;
    uint64_t round_robin = 0;
};
extern "C" int pqv_candidate_cursor_new(uint32_t file_count, pqv_candidate_cursor **out) {
    return guard([&] {
        if (!out) return fail(PQV_ERR_INVALID, "out must not be NULL");
        pqv_candidate_cursor *c = new pqv_candidate_cursor();
        c->candidates.resize(file_count);                                              // :202-206
        c->positions.assign(file_count, 0);
        *out = c;
        return static_cast<int>(PQV_OK);
    });
}
extern "C" int pqv_candidate_cursor_add(pqv_candidate_cursor *c, uint32_t idx, const uint32_t *rows, uint64_t n_rows) {
    return guard([&] {
        if (!c || (n_rows && !rows)) return fail(PQV_ERR_INVALID, "cursor/rows must not be NULL");
        if (idx < c->candidates.size()) c->candidates[idx].assign(rows, rows + n_rows);  // :209-213 (out of range: ignored)
        return static_cast<int>(PQV_OK);
    });
}
extern "C" int pqv_candidate_cursor_next_batch(pqv_candidate_cursor *c, uint64_t batch_size, uint32_t *out_file,
                                               uint32_t *out_row, uint64_t *n_out, uint64_t *per_file_taken) {
    return guard([&] {
        if (!c || !n_out || (batch_size && (!out_file || !out_row))) return fail(PQV_ERR_INVALID, "cursor/outputs must not be NULL");
        *n_out = 0;
        const uint64_t file_count = c->candidates.size();
        uint64_t n = 0;
        if (batch_size != 0 && file_count != 0) {                                      // :216-218
            uint64_t idx = c->round_robin;
            while (n < batch_size) {                                                   // :222-238
                bool progressed = false;
                for (uint64_t t = 0; t < file_count; ++t) {
                    const uint64_t f = idx % file_count;
                    idx += 1;
                    if (c->positions[f] < c->candidates[f].size()) {
                        out_file[n] = static_cast<uint32_t>(f);
                        out_row[n] = c->candidates[f][c->positions[f]++];
                        ++n;
                        progressed = true;
                        if (n >= batch_size) break;
                    }
                }
                if (!progressed) break;
            }
            c->round_robin = idx % file_count;                                         // :240
        }
        *n_out = n;
        if (per_file_taken) for (uint64_t f = 0; f < file_count; ++f) per_file_taken[f] = c->positions[f];
        return static_cast<int>(PQV_OK);
    });
}
extern "C" void pqv_candidate_cursor_free(pqv_candidate_cursor *c) { delete c; }

// ---------------------------------------------------------------------------------------
// batch-granular re-rank (update_topk_heap, src/df_vector/exec.rs:457-484)
// ---------------------------------------------------------------------------------------
// Scratch of the batch-granular re-rank, pooled per device: steady-state calls allocate nothing (the first version
// paid ten hipMallocs and six synchronous copies per 2048-row RecordBatch -- the allocation-bound pattern SURVEY D1
// criticises in row_to_scalar_values).  A context owns a private stream, device buffers grown on demand and pinned
// staging for the host-buffer entry point.
namespace {
struct RerankCtx {
    int device = 0;
    hipStream_t stream = nullptr;
    DevBuf d_cand, d_q, d_keys, d_vals, d_mvals, d_mdist, d_nf, d_saved, d_base, d_probe0, d_off, d_io_rows, d_io_d2, d_io_cnt, d_ids;
    PinnedBuf h_stage;
    uint64_t off_m = ~0ull, base_k = ~0ull;
    ~RerankCtx() { if (stream) (void)hipStreamDestroy(stream); }
};
std::mutex g_rerank_mu;
std::vector<RerankCtx *> g_rerank_pool;

int rerank_ctx_acquire(int device, RerankCtx **out) {
    {
        std::lock_guard<std::mutex> lock(g_rerank_mu);
        for (size_t i = 0; i < g_rerank_pool.size(); ++i)
            if (g_rerank_pool[i]->device == device) {
                *out = g_rerank_pool[i];
                g_rerank_pool.erase(g_rerank_pool.begin() + static_cast<long>(i));
                return PQV_OK;
            }
    }
    RerankCtx *c = new RerankCtx();
    c->device = device;
    hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e != hipSuccess) { delete c; return fail(PQV_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)); }
    *out = c;
    return PQV_OK;
}
void rerank_ctx_release(RerankCtx *c) {
    std::lock_guard<std::mutex> lock(g_rerank_mu);
    if (g_rerank_pool.size() < 16) g_rerank_pool.push_back(c); else delete c;
}

// The device-resident fold: d_cand [m, dim] and the running state all on the device; enqueued on `stream`.
int rerank_enqueue(RerankCtx &c, const float *d_query, const float *d_cand, const uint32_t *d_ids, uint64_t m, uint32_t dim,
                   uint32_t k_out, int metric, uint32_t *d_io_rows, float *d_io_d2, uint32_t *d_io_count, uint32_t *d_tie,
                   hipStream_t stream) {
    using namespace pqv;
    // with a tie flag the lists carry one extra entry (the runner-up), as pqv_topk_device_flags does
    const uint32_t k = d_tie ? k_out + 1 : k_out;
    const uint32_t bpl = static_cast<uint32_t>((m + 255) / 256);
    const uint32_t n_part = bpl * waves_per_block() + 1;  // +1: the running state
    HIP_TRY(c.d_keys.ensure(static_cast<size_t>(n_part) * k * sizeof(uint64_t)));
    HIP_TRY(c.d_vals.ensure(static_cast<size_t>(n_part) * k * sizeof(uint32_t)));
    HIP_TRY(c.d_mvals.ensure(k * sizeof(uint32_t)));
    HIP_TRY(c.d_mdist.ensure(k * sizeof(float)));
    HIP_TRY(c.d_nf.ensure(2 * sizeof(uint32_t)));
    HIP_TRY(c.d_saved.ensure(k * sizeof(uint32_t)));
    HIP_TRY(c.d_base.ensure(sizeof(uint64_t))); HIP_TRY(c.d_probe0.ensure(sizeof(uint32_t))); HIP_TRY(c.d_off.ensure(2 * sizeof(uint64_t)));
    if (c.off_m != m || c.base_k != k_out) {      // the one-list descriptor of the stream kernel (changes with the batch size only)
        const uint64_t h_base = k_out, h_off[2] = {0, m};
        const uint32_t h_probe0 = 0;
        c.off_m = ~0ull; c.base_k = ~0ull;        // nothing cached until all three copies have landed
        HIP_TRY(hipMemcpyAsync(c.d_base.p, &h_base, sizeof h_base, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(c.d_probe0.p, &h_probe0, sizeof h_probe0, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(c.d_off.p, h_off, sizeof h_off, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));        // the sources are stack variables
        c.off_m = m; c.base_k = k_out;
    }
    // running state as the first partial list: positions 0..count-1 (earlier arrivals win ties)
    HIP_TRY(launch_rerank_state_in(d_io_rows, d_io_d2, d_io_count, k_out, k, c.d_keys.as<uint64_t>(), c.d_vals.as<uint32_t>(),
                                   c.d_saved.as<uint32_t>(), stream));
    // batch candidates take positions k, k+1, ... via the cand_base entry
    StreamArgs ra{};
    ra.mat = d_cand; ra.row_of = nullptr; ra.list_off = c.d_off.as<uint64_t>();
    ra.probe = c.d_probe0.as<uint32_t>(); ra.cand_base = c.d_base.as<uint64_t>();
    ra.queries = d_query; ra.nq = 1; ra.nprobe = 1; ra.dim = dim; ra.k = k;
    ra.rows_per_block = 256; ra.blocks_per_list = bpl; ra.max_pos = ~0ull; ra.metric = metric;
    ra.part_keys = c.d_keys.as<uint64_t>() + k; ra.part_vals = c.d_vals.as<uint32_t>() + k;
    HIP_TRY(launch_stream(ra, STREAM_TOPK, stream));
    MergeArgs fm{};
    fm.part_keys = c.d_keys.as<uint64_t>(); fm.part_vals = c.d_vals.as<uint32_t>();
    fm.nq = 1; fm.n_part = n_part; fm.k_part = k; fm.k = k; fm.ids = nullptr;
    fm.row_idx = c.d_mvals.as<uint32_t>(); fm.dist = c.d_mdist.as<float>(); fm.n_found = c.d_nf.as<uint32_t>();
    fm.sqrt_out = 0; fm.k_out = k_out; fm.tie_flag = d_tie ? c.d_nf.as<uint32_t>() + 1 : nullptr;
    HIP_TRY(launch_merge_final(fm, stream));
    HIP_TRY(launch_rerank_state_out(c.d_mvals.as<uint32_t>(), c.d_mdist.as<float>(), c.d_nf.as<uint32_t>(), c.d_saved.as<uint32_t>(),
                                    d_ids, k_out, d_io_rows, d_io_d2, d_io_count, d_tie ? c.d_nf.as<uint32_t>() + 1 : nullptr, d_tie, stream));
    return PQV_OK;
}

int rerank_validate(const void *query, const void *io_rows, const void *io_d2, const void *io_count, const void *cand,
                    uint64_t m, uint32_t dim, uint32_t k, int metric) {
    if (!query || !io_rows || !io_d2 || !io_count) return fail(PQV_ERR_INVALID, "query/io arrays must not be NULL");
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");
    if (k > 1024) return fail(PQV_ERR_UNSUPPORTED, "k > 1024 is not supported");
    if (metric != PQV_L2SQ_REF4 && metric != PQV_L2SQ_SEQ) return fail(PQV_ERR_INVALID, "unknown metric");
    if (m && !cand) return fail(PQV_ERR_INVALID, "cand must not be NULL");
    if (m > 0x7FFFFFFFull) return fail(PQV_ERR_UNSUPPORTED, "batch larger than 2^31 rows");
    return PQV_OK;
}
}  // namespace

static int pqv_rerank_device_impl(int device, const void *d_query, const void *d_cand, const void *d_ids, uint64_t m,
                                  uint32_t dim, uint32_t k, int metric, void *d_io_rows, void *d_io_d2, void *d_io_count,
                                  void *d_tie_flag, void *hip_stream) {
    if (int rc = rerank_validate(d_query, d_io_rows, d_io_d2, d_io_count, d_cand, m, dim, k, metric)) return rc;
    if (d_tie_flag && k > 1023) return fail(PQV_ERR_UNSUPPORTED, "tie flags need a runner-up entry: k <= 1023");
    if (k == 0 || m == 0) return PQV_OK;
    if (int rc = use_device(device)) return rc;
    RerankCtx *c = nullptr;
    if (int rc = rerank_ctx_acquire(device, &c)) return rc;
    hipStream_t stream = hip_stream ? static_cast<hipStream_t>(hip_stream) : c->stream;
    int rc = rerank_enqueue(*c, static_cast<const float *>(d_query), static_cast<const float *>(d_cand),
                            static_cast<const uint32_t *>(d_ids), m, dim, k, metric, static_cast<uint32_t *>(d_io_rows),
                            static_cast<float *>(d_io_d2), static_cast<uint32_t *>(d_io_count), static_cast<uint32_t *>(d_tie_flag), stream);
    // the context's merge scratch is in use until the stream drains -- also when the enqueue failed half-way: hand it
    // back only then
    if (hipStreamSynchronize(stream) != hipSuccess && rc == PQV_OK) rc = fail(PQV_ERR_HIP, "hipStreamSynchronize failed");
    rerank_ctx_release(c);
    return rc;
}
extern "C" int pqv_rerank_device(int device, const void *d_query, const void *d_cand, const void *d_ids, uint64_t m,
                                 uint32_t dim, uint32_t k, int metric, void *d_io_rows, void *d_io_d2, void *d_io_count,
                                 void *hip_stream) {
    return guard([&] { return pqv_rerank_device_impl(device, d_query, d_cand, d_ids, m, dim, k, metric, d_io_rows, d_io_d2, d_io_count, nullptr, hip_stream); });
}
extern "C" int pqv_rerank_device_flags(int device, const void *d_query, const void *d_cand, const void *d_ids, uint64_t m,
                                       uint32_t dim, uint32_t k, int metric, void *d_io_rows, void *d_io_d2, void *d_io_count,
                                       void *d_tie_flag, void *hip_stream) {
    if (!d_tie_flag) return fail(PQV_ERR_INVALID, "d_tie_flag must not be NULL");
    return guard([&] { return pqv_rerank_device_impl(device, d_query, d_cand, d_ids, m, dim, k, metric, d_io_rows, d_io_d2, d_io_count, d_tie_flag, hip_stream); });
}

// Host-buffer fold with the reference's EXACT heap mechanics (exec.rs:457-484): the distances of the batch are
// computed on the GPU (stream_kernel, STREAM_DIST, in compute_distance_values' order), then the rows walk through
// std's BinaryHeap push / peek / pop on the host in arrival order -- an O(m) compare loop plus O(log k) per admitted
// row.  io_rows / io_d2 ARE the heap's backing array between batches, so ties (which make survivors and order depend
// on sift history) come out as in Rust; pqv_rerank_finish is heap.into_iter() + the stable sort of exec.rs:269-274.
template <class T>
static int rerank_host(int device, const float *query, const T *cand, const uint32_t *ids,
                       const uint8_t *valid, uint64_t m, uint32_t dim, uint32_t k, int metric,
                       uint32_t *io_rows, float *io_d2, uint32_t *io_count) {
    if (!query || !io_rows || !io_d2 || !io_count) return fail(PQV_ERR_INVALID, "query/io arrays must not be NULL");
    if (dim == 0) return fail(PQV_ERR_INVALID, "Embedding dimension must be > 0");
    if (metric != PQV_L2SQ_REF4 && metric != PQV_L2SQ_SEQ) return fail(PQV_ERR_INVALID, "unknown metric");
    if (m && !cand) return fail(PQV_ERR_INVALID, "cand must not be NULL");
    if (m > 0x7FFFFFFFull) return fail(PQV_ERR_UNSUPPORTED, "batch larger than 2^31 rows");
    if (k == 0) return PQV_OK;  // heap.len() < 0 is never true and peek() is None: nothing is kept
    if (*io_count > k) return fail(PQV_ERR_INVALID, "io_count exceeds k");
    if (m == 0) return PQV_OK;
    if (int rc = use_device(device)) return rc;
    uint64_t mv = m;
    if (valid) { mv = 0; for (uint64_t i = 0; i < m; ++i) mv += valid[i] != 0; }
    if (mv == 0) return PQV_OK;
    RerankCtx *c = nullptr;
    if (int rc = rerank_ctx_acquire(device, &c)) return rc;
    // the context goes back to the pool only with its stream drained (a failed call may have left work enqueued)
    struct Release { RerankCtx *c; ~Release() { (void)hipStreamSynchronize(c->stream); rerank_ctx_release(c); } } release{c};
    hipStream_t stream = c->stream;

    // pinned staging: [query | valid rows compacted in arrival order (null / wrong-length rows dropped, exec.rs:496-498,
    // 526-528), a Float64 column narrowed `as f32` on the way (exec.rs:542) | distances back]
    const size_t q_bytes = static_cast<size_t>(dim) * sizeof(float), c_bytes = static_cast<size_t>(mv) * dim * sizeof(float),
                 d_bytes = static_cast<size_t>(mv) * sizeof(float);
    HIP_TRY(c->h_stage.ensure(q_bytes + c_bytes + d_bytes + 64));
    uint8_t *hs = c->h_stage.as<uint8_t>();
    float *h_q = reinterpret_cast<float *>(hs), *h_c = reinterpret_cast<float *>(hs + q_bytes),
          *h_d = reinterpret_cast<float *>(hs + q_bytes + c_bytes);
    std::memcpy(h_q, query, q_bytes);
    {
        uint64_t o = 0;
        for (uint64_t i = 0; i < m; ++i) {
            if (valid && !valid[i]) continue;
            const T *src = cand + i * dim;
            float *dst = h_c + o * dim;
            if constexpr (std::is_same<T, float>::value) std::memcpy(dst, src, static_cast<size_t>(dim) * sizeof(float));
            else for (uint32_t j = 0; j < dim; ++j) dst[j] = static_cast<float>(src[j]);
            ++o;
        }
    }
    HIP_TRY(c->d_q.ensure(q_bytes)); HIP_TRY(c->d_cand.ensure(c_bytes)); HIP_TRY(c->d_mdist.ensure(d_bytes));
    HIP_TRY(c->d_base.ensure(sizeof(uint64_t))); HIP_TRY(c->d_probe0.ensure(sizeof(uint32_t))); HIP_TRY(c->d_off.ensure(2 * sizeof(uint64_t)));
    if (c->off_m != mv || c->base_k != 0) {       // the one-list descriptor of the stream kernel
        const uint64_t h_base = 0, h_off[2] = {0, mv};
        const uint32_t h_probe0 = 0;
        c->off_m = ~0ull; c->base_k = ~0ull;      // nothing cached until all three copies have landed
        HIP_TRY(hipMemcpyAsync(c->d_base.p, &h_base, sizeof h_base, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(c->d_probe0.p, &h_probe0, sizeof h_probe0, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipMemcpyAsync(c->d_off.p, h_off, sizeof h_off, hipMemcpyHostToDevice, stream));
        HIP_TRY(hipStreamSynchronize(stream));        // the sources are stack variables
        c->off_m = mv; c->base_k = 0;
    }
    HIP_TRY(hipMemcpyAsync(c->d_q.p, h_q, q_bytes, hipMemcpyHostToDevice, stream));
    HIP_TRY(hipMemcpyAsync(c->d_cand.p, h_c, c_bytes, hipMemcpyHostToDevice, stream));
    pqv::StreamArgs ra{};
    ra.mat = c->d_cand.as<float>(); ra.row_of = nullptr; ra.list_off = c->d_off.as<uint64_t>();
    ra.probe = c->d_probe0.as<uint32_t>(); ra.cand_base = c->d_base.as<uint64_t>();
    ra.queries = c->d_q.as<float>(); ra.nq = 1; ra.nprobe = 1; ra.dim = dim; ra.k = 1;
    ra.rows_per_block = 256; ra.blocks_per_list = static_cast<uint32_t>((mv + 255) / 256);
    ra.max_pos = ~0ull; ra.metric = metric; ra.out_f32 = c->d_mdist.as<float>();
    HIP_TRY(pqv::launch_stream(ra, pqv::STREAM_DIST, stream));
    HIP_TRY(hipMemcpyAsync(h_d, c->d_mdist.p, d_bytes, hipMemcpyDeviceToHost, stream));
    HIP_TRY(hipStreamSynchronize(stream));

    std::vector<HeapEnt> heap;
    heap.reserve(static_cast<size_t>(std::min<uint64_t>(k, static_cast<uint64_t>(*io_count) + mv)) + 1);     // sized by the data, not by a huge "keep everything" k
    for (uint32_t i = 0; i < *io_count; ++i) heap.push_back(HeapEnt{io_d2[i], io_rows[i]});     // the array IS the heap
    uint64_t o = 0;
    for (uint64_t i = 0; i < m; ++i) {
        if (valid && !valid[i]) continue;
        const HeapEnt ent{h_d[o++], ids ? ids[i] : static_cast<uint32_t>(i)};
        if (heap.size() < k) heap_push(heap, ent);                                     // exec.rs:474-475
        else if (ent.d < heap[0].d) { heap_pop(heap); heap_push(heap, ent); }          // :476-481
    }
    for (size_t i = 0; i < heap.size(); ++i) { io_rows[i] = heap[i].row; io_d2[i] = heap[i].d; }
    *io_count = static_cast<uint32_t>(heap.size());
    return PQV_OK;
}
extern "C" int pqv_rerank(int device, const float *query, const float *cand, const uint32_t *ids,
                          const uint8_t *valid, uint64_t m, uint32_t dim, uint32_t k, int metric,
                          uint32_t *io_rows, float *io_d2, uint32_t *io_count) {
    return guard([&] { return rerank_host<float>(device, query, cand, ids, valid, m, dim, k, metric, io_rows, io_d2, io_count); });
}
extern "C" int pqv_rerank_f64(int device, const float *query, const double *cand, const uint32_t *ids,
                              const uint8_t *valid, uint64_t m, uint32_t dim, uint32_t k, int metric,
                              uint32_t *io_rows, float *io_d2, uint32_t *io_count) {
    return guard([&] { return rerank_host<double>(device, query, cand, ids, valid, m, dim, k, metric, io_rows, io_d2, io_count); });
}
extern "C" int pqv_rerank_finish(const uint32_t *io_rows, const float *io_d2, uint32_t count, uint32_t *out_rows, float *out_d2) {
    return guard([&] {
        if (count && (!io_rows || !io_d2 || !out_rows || !out_d2)) return fail(PQV_ERR_INVALID, "state/output arrays must not be NULL");
        std::vector<HeapEnt> v(count);
        for (uint32_t i = 0; i < count; ++i) v[i] = HeapEnt{io_d2[i], io_rows[i]};     // heap.into_iter(): backing-array order
        std::stable_sort(v.begin(), v.end(), [](const HeapEnt &a, const HeapEnt &b) { return a.d < b.d; });   // exec.rs:270-274
        for (uint32_t i = 0; i < count; ++i) { out_rows[i] = v[i].row; out_d2[i] = v[i].d; }
        return static_cast<int>(PQV_OK);
    });
}

#ifdef PQV_STAMPS
// diagnostic build only (make stamps): device wall-clock stamps of the one-query launch sequence
extern "C" int pqv_debug_stamps(unsigned long long *out, int reset) {
    return pqv::stamps_io(out, reset) == hipSuccess ? 0 : -1;
}
#endif
