// Host runtime around the O(ND) kernels: packs ASCII sequences to the 2-bit pool,
// lays out per-task trace / ops regions in HBM, launches forward + traceback on one
// HIP stream, and hands column-kind streams back to the consensus engine.
//
// Buffers are grow-only and sized for MI355X's 288 GB HBM: a batch keeps every
// task's full trace (max_d rows x 16 B) resident, so there is no second pass and
// no host round trip between the forward sweep and the traceback.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <atomic>
#include <cassert>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <condition_variable>
#include <mutex>
#include <set>
#include <thread>
#include <type_traits>
#include <unordered_map>
#include <vector>

#include "nd_device.h"
#include "nd_host.h"
#include "nd_lqplan.h"
#include "nd_runtime.h"

namespace ndgpu {

namespace {

#define HIP_CHECK(expr)                                                                                       \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) {                                                                               \
            fprintf(stderr, "[ndgpu] HIP error %s at %s:%d: %s\n", hipGetErrorName(e_), __FILE__, __LINE__,   \
                    hipGetErrorString(e_));                                                                   \
            abort();                                                                                          \
        }                                                                                                     \
    } while (0)

static const bool g_debug_alloc = getenv("NDGPU_DEBUG_ALLOC") != nullptr;  // log every device buffer range (fault triage)
static const bool g_debug_launch = getenv("NDGPU_DEBUG_LAUNCH") != nullptr;  // triage: name + synchronise every launch group
#define NDGPU_DBG(st, ...)                                                                  \
    do {                                                                                    \
        if (g_debug_launch) {                                                               \
            (void)hipStreamSynchronize(st);                                                 \
            fprintf(stderr, "[ndgpu dbg %p] ", (void *)(st));                               \
            fprintf(stderr, __VA_ARGS__);                                                   \
            fprintf(stderr, "\n");                                                          \
            fflush(stderr);                                                                 \
        }                                                                                   \
    } while (0)
static std::mutex g_dbg_mu;  // NDGPU_DEBUG_LAUNCH=2: one device phase at a time over all contexts
static const bool g_debug_exclusive = getenv("NDGPU_DEBUG_LAUNCH") && atoi(getenv("NDGPU_DEBUG_LAUNCH")) >= 2;
static const bool g_debug_nofree = getenv("NDGPU_DEBUG_NOFREE") != nullptr;  // triage: outgrown buffers are leaked, not freed
// NDGPU_TRACE, read once per process: the "[ndgpu trace]" lines and run_extract's summary
static bool trace_on() { static const bool on = getenv("NDGPU_TRACE") != nullptr; return on; }
static uint64_t env_u64(const char *name, uint64_t unset) { return getenv(name) ? strtoull(getenv(name), nullptr, 10) : unset; }
static bool env_is(const char *name, const char *value) { return getenv(name) && !strcmp(getenv(name), value); }

// Test hook: NDGPU_OOM_ABOVE=bytes makes every device allocation larger than that fail as if the memory were exhausted.
static inline bool oom_injected(size_t bytes) {
    static const size_t lim = (size_t)env_u64("NDGPU_OOM_ABOVE", 0);
    return lim && bytes > lim;
}
// The same for the pinned host arenas: NDGPU_PINNED_OOM_ABOVE=bytes.
static inline bool oom_injected_pinned(size_t bytes) {
    static const size_t lim = (size_t)env_u64("NDGPU_PINNED_OOM_ABOVE", 0);
    return lim && bytes > lim;
}

static std::atomic<unsigned long long> g_reserved_bytes{0};  // kept free for the caller's other stage (ndgpu_reserve_device_memory)
static std::atomic<long long> g_dev_bytes{0};
// (re)allocations of device / pinned buffers since the last ndgpu_reset_stats and the wall time the calls took: an allocation in
// the middle of a step stalls every context (section 6 of DESIGN.md), so a steady-state step should show none
static std::atomic<unsigned long long> g_alloc_calls{0}, g_alloc_ns{0}, g_level_calls{0}, g_level_ns{0};
static std::atomic<int> g_leveling{0};  // level_buffers is at work (no kernel in flight): counted apart  // device memory held by the grow-only buffers of all contexts
// The runtime itself allocates on the device (kernel arguments, staging, scratch): a device filled to the last byte makes
// launches and copies fail where nothing can be done about it.  Allocations that would leave less than this are refused
// like an exhausted device (-> DeviceOom -> the sub-batch is halved).
constexpr size_t kDeviceHeadroom = (size_t)3 << 30;
static inline hipError_t guarded_malloc(void **p, size_t bytes) {
    if (oom_injected(bytes)) return hipErrorOutOfMemory;
    size_t free_b = 0, total_b = 0;
    if (bytes > ((size_t)64 << 20) && hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b < bytes + kDeviceHeadroom)
        return hipErrorOutOfMemory;
    return hipMalloc(p, bytes);
}

// The contexts pull their sub-batches from one queue, so a context may meet a larger sub-batch than it has seen while another
// context has met it before.  A buffer that has to grow therefore grows to the most ANY context has asked of the buffer of that
// name: after the first step or two every context holds the sizes of the largest sub-batch and nothing is (re)allocated in steady
// state -- a hipFree / hipHostMalloc in the middle of a step stalls every queue of the device (seconds, measured).
// A mark is recorded only AFTER an allocation of that size succeeded, and every mark is dropped when a context runs out of device
// memory (clear_high_water, from release_memory): a size that could not be had must not be asked for again by the halves of the
// sub-batch that failed (lib/nextcorrect.c:2254-2261: only a single pile that does not fit is an out-of-memory seed).
static std::mutex g_hw_mu;
static std::unordered_map<std::string, size_t> g_hw;
static size_t high_water(const char *name) {
    if (!name || !*name) return 0;
    std::lock_guard<std::mutex> lock(g_hw_mu);
    auto it = g_hw.find(name);
    return it == g_hw.end() ? 0 : it->second;
}
static void record_high_water(const char *name, size_t bytes) {
    if (!name || !*name) return;
    std::lock_guard<std::mutex> lock(g_hw_mu);
    size_t &v = g_hw[name];
    if (bytes > v) v = bytes;
}
static void clear_high_water() {
    std::lock_guard<std::mutex> lock(g_hw_mu);
    g_hw.clear();
}

struct AllocTimer {  // counts one (re)allocation and its wall time
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    ~AllocTimer() {
        const unsigned long long ns = (unsigned long long)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
        if (g_leveling.load()) g_level_calls++, g_level_ns += ns;
        else g_alloc_calls++, g_alloc_ns += ns;
    }
};

template <typename T>
struct DevBuf {
    T *p = nullptr;
    size_t cap = 0;
    const char *name = "";
    void reserve(size_t n) {
        if (n <= cap) return;
        const size_t asked = n;
        n = std::max(n, high_water(name) / sizeof(T));  // (what any context has HELD of this buffer; never a size that failed)
        const AllocTimer alloc_timer;
        if (p) {
            if (g_debug_alloc) fprintf(stderr, "[ndgpu alloc] free %s %p\n", name, (void *)p);
            if (!g_debug_nofree) HIP_CHECK(hipFree(p));
            g_dev_bytes -= (long long)(cap * sizeof(T));
        }
        p = nullptr;
        cap = 0;
        // most wanted first: the mark with growth slack, the mark, what this call needs with slack, what this call needs
        size_t want = 0;
        hipError_t rc = hipErrorOutOfMemory;
        const size_t tries[4] = {n + n / 4 + 1024, n + 1024, asked + asked / 4 + 1024, asked + 1024};
        for (int t = 0; t < 4 && rc == hipErrorOutOfMemory; t++) {
            if (t && tries[t] >= want) continue;
            want = tries[t];
            rc = guarded_malloc((void **)&p, want * sizeof(T));
        }
        if (rc == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            p = nullptr;
            throw DeviceOom{want * sizeof(T)};
        }
        HIP_CHECK(rc);
        cap = want;
        record_high_water(name, std::min(want - 1024, n) * sizeof(T));
        g_dev_bytes += (long long)(cap * sizeof(T));
        if (g_debug_alloc)
            fprintf(stderr, "[ndgpu alloc] %s %p .. %p (%zu bytes, asked %zu)\n", name, (void *)p, (void *)((char *)p + want * sizeof(T)),
                    want * sizeof(T), asked * sizeof(T));
    }
    void release() {
        if (p) {
            (void)hipFree(p);
            g_dev_bytes -= (long long)(cap * sizeof(T));
        }
        p = nullptr;
        cap = 0;
    }
    ~DevBuf() { release(); }
};

template <typename T>
struct PinBuf {
    T *p = nullptr;
    size_t cap = 0;
    const char *name = "";
    void reserve(size_t n) {
        if (n <= cap) return;
        const size_t asked = n;
        n = std::max(n, high_water(name) / sizeof(T));
        const AllocTimer alloc_timer;
        if (p && !g_debug_nofree) HIP_CHECK(hipHostFree(p));
        p = nullptr;
        cap = 0;
        size_t want = n + n / 4 + 1024;
        hipError_t rc = oom_injected_pinned(want * sizeof(T)) ? hipErrorOutOfMemory : hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
        if (rc == hipErrorOutOfMemory && asked + 1024 < want) {  // what this call needs, no more
            (void)hipGetLastError();
            want = asked + 1024;
            rc = oom_injected_pinned(want * sizeof(T)) ? hipErrorOutOfMemory : hipHostMalloc((void **)&p, want * sizeof(T), hipHostMallocDefault);
        }
        if (rc == hipErrorOutOfMemory) {
            (void)hipGetLastError();
            p = nullptr;
            throw DeviceOom{want * sizeof(T)};
        }
        HIP_CHECK(rc);
        cap = want;
        record_high_water(name, std::min(want - 1024, n) * sizeof(T));
        if (g_debug_alloc) fprintf(stderr, "[ndgpu alloc] pinned %p .. %p\n", (void *)p, (void *)((char *)p + want * sizeof(T)));
    }
    void release() {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    ~PinBuf() { release(); }
};

struct CodeLut {
    uint8_t v[256];
    CodeLut() {
        memset(v, 0xff, sizeof(v));
        v['A'] = 0;
        v['C'] = 1;
        v['G'] = 2;
        v['T'] = 3;
    }
};
const CodeLut kCode;

// ASCII [ACGT]* -> 2-bit, LSB-first, into a preallocated word range.  Returns false on any other byte (the reference compares raw
// bytes; we only accept what lib/bseq.c can emit from a .2bit DB).
bool pack_into(uint32_t *out, const char *s, size_t n) {
    unsigned bad = 0;
    size_t i = 0, w = 0;
    for (; i + 16 <= n; w++, i += 16) {
        uint32_t acc = 0;
        for (int b = 0; b < 16; b++) {
            const uint8_t c = kCode.v[(unsigned char)s[i + b]];
            bad |= c;
            acc |= (uint32_t)(c & 3u) << (2 * b);
        }
        out[w] = acc;
    }
    if (i < n) {
        uint32_t acc = 0;
        for (int b = 0; i + b < n; b++) {
            const uint8_t c = kCode.v[(unsigned char)s[i + b]];
            bad |= c;
            acc |= (uint32_t)(c & 3u) << (2 * b);
        }
        out[w] = acc;
    }
    return (bad & 0x80u) == 0;
}
// The same, appended to a pool at a word boundary.
bool pack_append(std::vector<uint32_t> &pool, const char *s, size_t n) {
    const size_t w0 = pool.size();
    pool.resize(w0 + (n + 15) / 16);
    return pack_into(pool.data() + w0, s, n);
}

// Every grow-only buffer of a context, once: X(element type, member, device | pinned, levelled | on_demand).  The members of State, their
// names (the strings key the high-water marks and are shared by all contexts), release_memory's releases and level_buffers' pass are all
// generated from this list, in this order.
//   device | pinned: a DevBuf in HBM or a PinBuf of page-locked host memory (level_buffers charges only device growth to its budget)
//   on_demand: reserved only by the sub-batch that needs it and therefore never levelled -- bringing it up to another context's mark
//   would spend device memory in every context on a path most sub-batches never take; levelled: everything else
enum class BufPlace { device, pinned };
enum class BufLevel { levelled, on_demand };
#define NDGPU_BUFFERS(X)                                                                                                                  \
    /* low-quality-region rounds (K12) */                                                                                                 \
    X(LqPileDev, d_lq_piles, device, levelled)                                                                                            \
    X(LqPieceDev, d_lq_pieces, device, levelled)                                                                                          \
    X(uint32_t, d_lq_rec, device, levelled)                                                                                               \
    X(LqJobDev, d_lq_jobs, device, levelled) /* K12a's jobs and their streams: a header per cell row, a word per link */                  \
    X(uint64_t, d_lq_hdr, device, levelled)                                                                                               \
    X(uint32_t, d_lq_lnk, device, levelled)                                                                                               \
    X(char, d_lq_out, device, levelled) /* the piles' characters / the jobs' stretches of the walk (one slot per cell row) */             \
    X(char, d_lq_tmp, device, levelled)                                                                                                   \
    X(int32_t, d_lq_bnd, device, levelled) /* K12b's boundary planes: 4 x kLqLinkCap words per job */                                     \
    /* POA (K13): jobs, the ids each kernel form takes, query bytes, rows, predecessor rows, scores, origins, routes */                    \
    X(PoaJobDev, d_poa_jobs, device, levelled)                                                                                            \
    X(uint32_t, d_poa_ids, device, levelled)                                                                                              \
    X(char, d_poa_q, device, levelled)                                                                                                    \
    X(PoaRowDev, d_poa_rows, device, levelled)                                                                                            \
    X(uint16_t, d_poa_preds, device, levelled)                                                                                            \
    X(int32_t, d_poa_s, device, levelled)                                                                                                 \
    X(uint16_t, d_poa_f, device, levelled)                                                                                                \
    X(uint32_t, d_poa_route, device, levelled)                                                                                            \
    /* resident POA graphs (K19): problems, sequence table, the round's problems, X and error word per problem, strings; the arenas */     \
    X(PoaGraphDev, d_poa_graphs, device, levelled)                                                                                        \
    X(PoaSeqDev, d_poa_seqs, device, levelled)                                                                                            \
    X(PoaRoundDev, d_poa_round, device, levelled)                                                                                         \
    X(PoaXeDev, d_poa_xe, device, levelled)                                                                                               \
    X(uint32_t, d_poa_out, device, levelled)                                                                                              \
    X(uint64_t, d_poa_arena, device, on_demand) /* only under NDGPU_POA_RESIDENT=1 / the flags entry: never levelled */                   \
    /* forward / traceback (K7 / K8a) */                                                                                                  \
    X(uint32_t, d_pool, device, levelled)                                                                                                 \
    X(uint32_t, d_ops, device, levelled)                                                                                                  \
    X(AlnTask, d_tasks, device, levelled)                                                                                                 \
    X(AlnOut, d_outs, device, levelled)                                                                                                   \
    X(uint64_t, d_trace, device, levelled)                                                                                                \
    X(int32_t, d_v, device, levelled)                                                                                                     \
    /* wide-band alignments (K7w): trace rows and their min_k -- members, not locals of run_wide: a local buffer was a hipMalloc +        \
       hipFree per call, and hipFree waits for every stream of the device */                                                              \
    X(uint64_t, d_wtrace, device, levelled)                                                                                               \
    X(int32_t, d_wmink, device, levelled)                                                                                                 \
    X(AlnTask, d_wtasks, device, levelled) /* the wide tasks' records of one group, in list order (one upload, not one per task) */       \
    /* segmented traceback (ond_kernels.hip): checkpoint cells / headers the forward kernel leaves, the walkers and what they report */   \
    X(uint32_t, d_ck_cells, device, levelled)                                                                                             \
    X(uint2, d_ck_hdr, device, levelled)                                                                                                  \
    X(TbSeg, d_tbseg, device, levelled)                                                                                                   \
    X(TbSegOut, d_tbout, device, levelled)                                                                                                \
    X(int32_t, d_ids, device, levelled)                                                                                                   \
    /* K15 (align_batch_runs): per-task summaries, the bad-task bits, the runs' offsets, the runs (exact size, never n_cols a task) */     \
    X(AlnRunSum, d_run_sums, device, levelled)                                                                                            \
    X(uint32_t, d_run_skip, device, levelled)                                                                                             \
    X(uint64_t, d_run_off, device, levelled)                                                                                              \
    X(uint32_t, d_runs, device, levelled)                                                                                                 \
    /* main phase (alive from run_main to end_batch) */                                                                                   \
    X(ReadDev, d_reads, device, levelled)                                                                                                 \
    X(PileDev, d_piles, device, levelled)                                                                                                 \
    X(uint32_t, d_read_pile, device, levelled)                                                                                            \
    X(uint32_t, d_acc, device, levelled)                                                                                                  \
    X(uint32_t, d_tags, device, levelled)                                                                                                 \
    X(uint32_t, d_colidx, device, levelled)                                                                                               \
    X(uint32_t, d_cov, device, levelled) /* coverage | insertion counts | longest insertion: one block, one fill */                       \
    X(uint32_t, d_cellbase, device, levelled)                                                                                             \
    X(uint32_t, d_entbase, device, levelled)                                                                                              \
    X(uint32_t, d_cell_start, device, levelled)                                                                                           \
    X(uint32_t, d_cell_len, device, levelled)                                                                                             \
    X(uint32_t, d_cell_bpp, device, levelled)                                                                                             \
    X(uint32_t, d_cell_blink, device, levelled)                                                                                           \
    X(uint32_t, d_ent_pp, device, levelled)                                                                                               \
    X(uint32_t, d_ent_ppp, device, levelled)                                                                                              \
    X(uint32_t, d_ent_cnt, device, levelled)                                                                                              \
    X(uint32_t, d_err, device, levelled)                                                                                                  \
    X(long long, d_ent_score, device, on_demand) /* the int64 scoring kernel's 8 bytes per link: only when a pile needs that kernel */    \
    X(uint32_t, d_link_lists, device, on_demand) /* K9's third attempt: allocated only when a sub-batch needs it */                       \
    X(int32_t, d_cell_best, device, levelled) /* K10 segments: cell bests, boundary scores (kSegEnts per segment) */                      \
    X(int32_t, d_spec, device, levelled)                                                                                                  \
    X(int32_t, d_fin, device, levelled)                                                                                                   \
    X(SegSum, d_sums, device, levelled)                                                                                                   \
    X(SegItem, d_items, device, levelled)                                                                                                 \
    X(uint32_t, d_bt_exit, device, levelled) /* best_pp walk by segments */                                                               \
    X(uint32_t, d_bt_steps, device, levelled)                                                                                             \
    X(uint32_t, d_bt_entry, device, levelled)                                                                                             \
    X(uint32_t, d_bt_off, device, levelled)                                                                                               \
    X(PathItem, d_path, device, levelled)                                                                                                 \
    X(ColBlock, d_blocks, device, levelled)                                                                                               \
    /* K20: jobs, result records, a word per path slot, window slots, the dense words and windows that come down */                       \
    X(CnsJobDev, d_cns_jobs, device, levelled)                                                                                            \
    X(CnsOutDev, d_cns_out, device, levelled)                                                                                             \
    X(uint32_t, d_cns_words, device, levelled)                                                                                            \
    X(uint32_t, d_cns_wins, device, levelled)                                                                                             \
    X(uint32_t, d_cns_dense, device, levelled)                                                                                            \
    X(uint32_t, d_cns_wdense, device, levelled)                                                                                           \
    /* K21 (words, windows and their dense forms are K20's buffers: a launch runs one of the two): jobs, result records, a character */  \
    /* per path slot, the dense strings that come down, the seeds' byte codes of the batched entry */                                     \
    X(CnsWalkJobDev, d_cnsw_jobs, device, levelled)                                                                                       \
    X(CnsWalkOutDev, d_cnsw_out, device, levelled)                                                                                        \
    X(uint8_t, d_cnsw_chars, device, levelled)                                                                                            \
    X(uint8_t, d_cnsw_seq, device, levelled)                                                                                              \
    X(uint8_t, d_cnsw_seed, device, levelled)                                                                                             \
    /* K24: jobs, regions, words, pseudo-seed bytes, a slice of emitted characters per job, result records, the dense strings */          \
    X(SpliceJobDev, d_splice_jobs, device, levelled)                                                                                      \
    X(SpliceRegDev, d_splice_regs, device, levelled)                                                                                      \
    X(uint32_t, d_splice_words, device, levelled)                                                                                         \
    X(uint8_t, d_splice_seeds, device, levelled)                                                                                          \
    X(uint8_t, d_splice_chars, device, levelled)                                                                                          \
    X(SpliceOutDev, d_splice_out, device, levelled)                                                                                       \
    X(uint8_t, d_splice_seq, device, levelled)                                                                                            \
    X(RegionDev, d_regions, device, levelled)                                                                                             \
    X(char, d_strpool, device, levelled)                                                                                                  \
    X(unsigned long long, d_cursor, device, levelled)                                                                                     \
    /* K22: the piles that ask, a record and the work words per region of the launch -- only in launches with such a pile */             \
    X(PhasePileDev, d_phase_piles, device, levelled)                                                                                      \
    X(PhaseRegionDev, d_phase_out, device, levelled)                                                                                      \
    X(uint32_t, d_phase_work, device, levelled)                                                                                           \
    /* host side: run_chunk's ops and every caller's AlnOut records; the two transfer arenas (see State::h2d / d2h) */                    \
    X(uint32_t, h_ops, pinned, levelled)                                                                                                  \
    X(AlnOut, h_outs, pinned, levelled)                                                                                                   \
    X(char, up, pinned, levelled)                                                                                                         \
    X(char, down, pinned, levelled)

// One launch of the forward / traceback pair: tasks [begin, end) of a context's table (plan_chunks)
struct AlignChunk {
    size_t begin, end;
    bool seg;        // the traceback runs in segments (tb_assign)
    uint64_t slots;  // walker slots of the launch (0 unless seg)
};

// The main phase's results, step by step (run_main).  What layout_piles makes of a sub-batch beside the context's pool, tasks, reads
// and piles: the pile of every read, the piles with a byte outside [ACGT], and the slot totals the buffers are sized by.
struct MainLayout {
    std::vector<uint32_t> read_pile;
    std::vector<uint8_t> bad_pile;
    uint64_t ops_words = 0, tag_slots = 0, colidx_slots = 0, col_slots = 0, acc_slots = 0;
};
constexpr uint64_t kTagSlotLimit = 1ull << 32;  // count_links keeps a read's tag base (ReadDev::tag_off) in 32 bits
struct CovPlanes {  // d_cov's three arrays of col_slots + 1 words: coverage, insertion count, longest insertion
    uint32_t *cov, *inscnt, *insmax;
};
struct MsaPlan {  // plan_msa: K10's work lists by tier, K9's column blocks, the totals of cells / links / path items / segments
    std::vector<SegItem> items_small, items_large, items_slow;  // (slow: piles of the int64 kernel; only the walk uses them)
    std::vector<ColBlock> blocks;
    uint64_t cells = 0, ents = 0, paths = 0;
    uint32_t n_segs = 0;
    size_t n_items() const { return items_small.size() + items_large.size() + items_slow.size(); }
};
struct MsaResult {  // count_and_score: the last attempt's error words, its piles, its paths (a view into the download arena)
    uint32_t herr[kErrWords] = {};
    const PathItem *hpath = nullptr;   // (nullptr where K20 took the walks: MsaResult::cns)
    std::vector<PileDev> piles;
    std::vector<CnsOutDev> cns;        // K20's records, one per pile
    std::vector<CnsWalkOutDev> cnsw;   // or K21's (CnsPlan::walk)
};
struct SplicePack {                        // one launch of run_splice: the jobs it takes (ids into the requests) and their arenas
    std::vector<SpliceJobDev> jobs;
    std::vector<SpliceRegDev> regs;
    std::vector<uint32_t> words;
    std::vector<uint8_t> seeds;
    std::vector<size_t> ids;
    uint64_t chars = 0;
};
struct CnsPlan {  // plan_cns: K20's jobs of a launch (one per pile, or per walk of run_cns) and the window slots they share
    std::vector<CnsJobDev> jobs;
    uint64_t win_slots = 0;
    bool walk = false;                 // a pile of the launch is HiFi or -fast: K21 takes the launch, its jobs are wjobs
    std::vector<CnsWalkJobDev> wjobs;
    bool any_hifi = false, any_fast = false;
};

struct LqSrc {  // a sequence of an LQ call's pool: packed already (words), or ASCII
    const uint32_t *words;
    const char *ascii;
    uint32_t len;
    uint64_t word_off;
};
struct LqLayout {  // layout_lq: per round its device record and whether K12 takes it; the pieces, jobs and sequences of all rounds; the totals
    std::vector<LqPileDev> piles;
    std::vector<uint8_t> usable;
    std::vector<LqPieceDev> pieces;
    std::vector<LqJobDev> jobs;
    std::vector<LqSrc> srcs;
    uint64_t pool_words = 0, ops_words = 0, cell_rows = 0, out_bytes = 0, hdr_words = 0, lnk_words = 0;
};
struct PoaProb {
    PoaGraph g;
    PoaRows rows;
    bool live = false;   // still on the device path
    uint64_t cells = 0;  // of the round in progress
    uint32_t job = 0;    // its job of the launch in progress
};
struct PoaBatch {  // run_poa: the problems, and the launch in progress -- its five staged tables, what it sizes, what comes back
    std::vector<PoaProb> probs;
    std::vector<PoaJobDev> jobs;
    std::vector<PoaRowDev> rows;
    std::vector<uint16_t> preds;
    std::vector<char> qpool;
    std::vector<uint32_t> ids, routes;  // ids: the wave form's jobs [0, n_wave), then the workgroup form's
    size_t n_wave = 0;
    uint64_t cells = 0, route_words = 0;
    explicit PoaBatch(size_t n) : probs(n) {}
};
struct PoaResident {  // run_poa's resident form: the problems whose graphs live on the device, index p = its place in every table
    std::vector<size_t> req;            // p -> the request
    std::vector<PoaGraphDev> graphs;
    std::vector<PoaSeqDev> seqs;
    std::vector<char> pool;             // every sequence, a NUL behind each
    std::vector<PoaXeDev> xe;           // as the last round left them (X of a start chain = its length)
    std::vector<uint8_t> live;          // still on the resident path
    uint64_t arena_bytes = 0, out_bytes = 0;
    size_t max_seqs = 0;
    // the round in progress: its problems in launch order, the ids each launch's two forms take, the launches
    std::vector<PoaRoundDev> round;
    std::vector<uint32_t> ids;
    struct Launch { size_t first, n_wave, n_group; uint64_t cells; };
    std::vector<Launch> launches;
};

}  // namespace

static inline double ms_between(hipEvent_t a, hipEvent_t b) {  // HIP-event time from a to b (both reached)
    float ms = 0;
    HIP_CHECK(hipEventElapsedTime(&ms, a, b));
    return ms;
}

struct DeviceAligner::State {
    int device = 0;
    const uint32_t *db_pool = nullptr;  // resident read DB of the batch in progress (owned by its ndgpu_db handle)
    hipStream_t stream = nullptr, lat_stream = nullptr;  // lat_stream: reserved compute units (see the constructor)
    hipStream_t stream2 = nullptr;                        // scoring launch of the piles that need the large LDS tables
    hipEvent_t ev_lat0 = nullptr, ev_lat1 = nullptr, ev_fork = nullptr, ev_join = nullptr;
    int reserved_cus = 0;
    std::mutex mu;
#define NDGPU_MEMBER(T, x, place, level) std::conditional_t<BufPlace::place == BufPlace::device, DevBuf<T>, PinBuf<T>> x;
    NDGPU_BUFFERS(NDGPU_MEMBER)
#undef NDGPU_MEMBER
    std::vector<int32_t> order;
    std::vector<uint32_t> order_cls;
    // Held from begin_batch to end_batch.  Not a plain mutex: with two batch calls in flight (the caller's pipeline: the tail of one
    // call under the main phases of the next) the context must serve the OLDER call's sub-batches first, whichever thread asked first.
    struct OrderedLock {
        std::mutex m;
        std::condition_variable cv;
        bool held = false;
        std::multiset<uint64_t> waiting;
        // reserved: the caller holds a reservation of this order (reserve()): its place in the line stays taken between its batches, so
        // a newer call's thread that is already waiting does not slip in while the older call's thread fetches its next sub-batch
        void lock(uint64_t order = 0, bool reserved = false) {
            std::unique_lock<std::mutex> l(m);
            if (reserved && waiting.find(order) == waiting.end()) reserved = false;  // (no such reservation: waits like any other caller)
            auto it = reserved ? waiting.end() : waiting.insert(order);
            cv.wait(l, [&] { return !held && !waiting.empty() && *waiting.begin() == order; });
            if (!reserved) waiting.erase(it);
            held = true;
        }
        void reserve(uint64_t order) {
            std::lock_guard<std::mutex> l(m);
            waiting.insert(order);
        }
        void unreserve(uint64_t order) {
            {
                std::lock_guard<std::mutex> l(m);
                auto it = waiting.find(order);
                if (it != waiting.end()) waiting.erase(it);
            }
            cv.notify_all();
        }
        void unlock() {
            {
                std::lock_guard<std::mutex> l(m);
                held = false;
            }
            cv.notify_all();
        }
        bool try_lock() {
            std::lock_guard<std::mutex> l(m);
            if (held || !waiting.empty()) return false;
            held = true;
            return true;
        }
    } batch_mu;
    std::vector<ReadDev> reads;  // main-phase state (alive from run_main to end_batch)
    std::vector<PileDev> piles;
    // The context's timing events, each named by the one step that records it; read with ms() behind a synchronisation.
    enum Ev {
        kEvFrontK7, kEvFrontK8a,                                 // chunk_front: before K7 | between K7 and K8a
        kEvMainK7, kEvMainK8a, kEvMainAligned,                   // align_main, chunk by chunk: before K7 | K8a | behind it
        kEvTagsBegin, kEvTagsEnd,                                // launch_tags: around its four launches
        kEvLinksBegin, kEvScoreBegin, kEvWalkBegin, kEvWalkEnd,  // count_and_score, score_pass: before K9 | K10 | the walk | behind it
        kEvLqMsaBegin, kEvLqMsaEnd,                              // launch_lq: around K12 (its K7 / K8a: lq_evs)
        kEvTailBegin, kEvTailEnd, kEvExtractRanked,  // K11, K13, K14, K15: around the launch in flight | behind K14 where it follows K11
        kEvPoaRows, kEvPoaAlign, kEvPoaThread, kEvPoaEnd,  // a resident POA round: before K19's rows | K13's launches | K19's thread | behind it
        kEvCnsBegin, kEvCnsEnd,                            // launch_cns: around K20 and its gather
        kEvCnswBegin, kEvCnswEnd,                          // launch_cns_walk: around K21 and its gather
        kEvPhaseBegin, kEvPhaseEnd,                        // phase_on_pool: around K22's two kernels
        kEvSpliceBegin, kEvSpliceEnd,                      // launch_splice_jobs: around K24 and its gather
        kEvCount
    };
    hipEvent_t evs[kEvCount] = {nullptr};
    std::vector<hipEvent_t> lq_evs;  // launch_lq: K7 / K8a brackets per chunk (a chunk count is not bounded)
    void mark(Ev e, hipStream_t st) { HIP_CHECK(hipEventRecord(evs[e], st)); }
    double ms(Ev a, Ev b) const { return ms_between(evs[a], evs[b]); }
    std::vector<uint32_t> pool;
    std::vector<AlnTask> tasks;
    RuntimeStats stats;
    size_t trace_budget_bytes = (size_t)48 << 30;
    int host_threads = 1;
    uint64_t k9_retries = 0;

    // Host <-> device transfers go through two pinned arenas of the context (up, down).  An asynchronous copy from / to pageable
    // memory makes the runtime pin the caller's pages for the duration of the copy; with eight contexts doing that at
    // the same time from neighbouring heap blocks, one context's unpin took a page another context's copy was still
    // using (GPU memory access faults on host heap addresses).  Everything a kernel or a copy engine touches is now
    // either device memory or these arenas.
    size_t up_used = 0, down_used = 0;
    struct Pending {
        void *dst;
        size_t off, bytes;
    };
    std::vector<Pending> pending;
    void drain() {  // the stream is idle: hand the downloaded bytes to their owners, recycle both arenas
        for (const Pending &q : pending) memcpy(q.dst, down.p + q.off, q.bytes);
        pending.clear();
        up_used = down_used = 0;
    }
    void sync_drain(hipStream_t st) {
        HIP_CHECK(hipStreamSynchronize(st));
        drain();
    }
    void reserve_down(size_t bytes, hipStream_t st) {  // room for `bytes` of downloads without moving the arena (views stay valid)
        if (down_used + bytes + 4096 <= down.cap) return;
        sync_drain(st);
        down.reserve(bytes + 4096);
    }
    void h2d(void *dst, const void *src, size_t bytes, hipStream_t st) {
        if (!bytes) return;
        const size_t need = (bytes + 255) & ~(size_t)255;
        if (up_used + need > up.cap) {
            sync_drain(st);
            up.reserve(std::max(need, up.cap * 2));
        }
        memcpy(up.p + up_used, src, bytes);
        HIP_CHECK(hipMemcpyAsync(dst, up.p + up_used, bytes, hipMemcpyHostToDevice, st));
        up_used += need;
    }
    // device -> host: the bytes land in the arena; dst_host (if given) receives them at the next drain; the returned
    // pointer is valid from the next stream synchronisation until the next drain / reserve
    void *d2h(void *dst_host, const void *src_dev, size_t bytes, hipStream_t st) {
        const size_t need = (bytes + 255) & ~(size_t)255;
        if (down_used + need > down.cap) {
            sync_drain(st);
            down.reserve(std::max(need, down.cap * 2));
        }
        char *at = down.p + down_used;
        if (bytes) HIP_CHECK(hipMemcpyAsync(at, src_dev, bytes, hipMemcpyDeviceToHost, st));
        if (dst_host && bytes) pending.push_back(Pending{dst_host, down_used, bytes});
        down_used += need;
        return at;
    }

    // What every device phase of a context starts with, in this order: the lock of NDGPU_DEBUG_LAUNCH=2 (one phase at a time over
    // all contexts), the context's own lock, the context's device.
    struct Phase {
        std::unique_lock<std::mutex> dbg;
        std::lock_guard<std::mutex> lock;
        explicit Phase(State &S) : dbg(g_debug_exclusive ? std::unique_lock<std::mutex>(g_dbg_mu) : std::unique_lock<std::mutex>()), lock(S.mu) {
            HIP_CHECK(hipSetDevice(S.device));
        }
    };

    // The forward / traceback ("align") phase that run_chunk, run_lq and run_main share (defined with the traceback's set-up below)
    std::vector<AlignChunk> plan_chunks(AlnTask *t, size_t nt);
    void launch_chunk(const AlignChunk &c, const int32_t *order, const int32_t *tb_order, hipEvent_t ev_mid, hipEvent_t ev_end, const char *who);
    void tally_outs(size_t nt, std::vector<int32_t> *wide);
    void run_wide(bool ops_to_host, const std::vector<int32_t> &ids);  // the tasks whose live band left the register path, again with V in HBM

    // The steps of run_main, in its order (defined above it)
    MainLayout layout_piles(MainPile **mp, size_t np);
    void reserve_layout(const MainLayout &L, size_t np);
    const int32_t *length_order(size_t a, size_t m);
    void align_main(const std::vector<AlignChunk> &chunks, size_t np);
    void launch_tags(const CovPlanes &cov, size_t np);
    void upload_plan(const MsaPlan &plan);
    MsaResult count_and_score(const MsaPlan &plan, const CovPlanes &cov, const CnsPlan *cns);
    CnsPlan plan_cns(const MsaPlan &plan, MainPile **mp);
    void launch_cns(const CnsPlan &cns, const PileDev *dev_piles, const PathItem *dev_path);
    void fetch_cns(const CnsPlan &cns, const MsaResult &res, const std::vector<uint8_t> &bad_pile, MainPile **mp);
    CnsPlan plan_cns_walk(const MsaPlan &plan, MainPile **mp);
    void reserve_cns_walk(const CnsPlan &cns, size_t slots);
    void launch_cns_walk_jobs(const CnsPlan &cns, const PileDev *dev_piles, const PathItem *dev_path);
    void fetch_cns_walk(const CnsPlan &cns, const MsaResult &res, const std::vector<uint8_t> &bad_pile, MainPile **mp);
    // The steps of run_splice, in its order (defined above it)
    size_t pack_splice(SpliceReq **reqs, size_t a, size_t n, SplicePack &P);
    void launch_splice_jobs(const SplicePack &P);
    void fetch_splice(SpliceReq **reqs, const SplicePack &P);
    void score_pass(const MsaPlan &plan, const K10Args &k10);
    void rescue_pass(const MsaPlan &plan, const K10Args &k10);
    void k9_digest_trace(const K9Args &k9, size_t np);
    void tally_main(const MsaPlan &plan, const std::vector<uint8_t> &bad_pile, MainPile **mp, const uint64_t tp[5]);

    // The steps of run_lq, run_poa and run_extract, in their order (defined above each)
    LqLayout layout_lq(LqRound **rounds, size_t n);
    void layout_lq_round(LqRound &R, size_t r, LqLayout &L);
    bool pack_lq_pool(const LqLayout &L);
    std::vector<AlignChunk> reserve_lq(const LqLayout &L);
    std::vector<char> launch_lq(LqLayout &L, const std::vector<AlignChunk> &chunks);
    void tally_lq(LqRound **rounds, const LqLayout &L, size_t n_chunks, const std::vector<char> &out);
    void grow_lq_evs(size_t n) { for (hipEvent_t e; lq_evs.size() < n; lq_evs.push_back(e)) HIP_CHECK(hipEventCreate(&e)); }
    size_t admit_poa(PoaReq **reqs, size_t n, uint64_t budget, PoaBatch &B);
    void export_rows(PoaBatch &B, PoaReq **reqs, const std::vector<size_t> &ids, size_t r, std::vector<PoaLoad> &load);
    void stage_poa_slice(PoaBatch &B, PoaReq **reqs, const std::vector<size_t> &slice, size_t r);
    void launch_poa_slice(PoaBatch &B, size_t r);
    void thread_routes(PoaBatch &B, PoaReq **reqs, const std::vector<size_t> &slice, size_t r);
    void poa_rounds(PoaReq **reqs, size_t n);    // run_poa's two forms: K13's rounds with the graphs on the host | resident graphs (K19)
    void poa_resident(PoaReq **reqs, size_t n);
    void admit_poa_resident(PoaReq **reqs, size_t n, uint64_t budget, PoaResident &R, std::vector<PoaReq *> &rest);
    void start_poa_graphs(PoaResident &R);
    void poa_resident_round(PoaResident &R, PoaReq **reqs, size_t r, uint64_t budget);
    void poa_resident_consensus(PoaResident &R, PoaReq **reqs);
    template <typename F>
    void poa_each(const std::vector<size_t> &ids, F f) {  // f(problem) over the context's host threads
        host_each(ids.size(), ids.size() < 8 || host_threads <= 1, host_threads, ids.size() / 4, true, [&](size_t k) { f(ids[k]); });
    }
    unsigned extract_into_pool(std::vector<RegionDev> &regs, bool rank, std::vector<char> &hstr);
    void phase_on_pool(std::vector<PhasePileDev> &pp, std::vector<PhaseRegionDev> &recs, size_t n_regions, size_t pool_cap, const char *who);
};

static int g_ctx_creating = -1;  // index of the context under construction (guarded by g_ctx_mu)

DeviceAligner::DeviceAligner() : s_(new State) {
    // every context drives its own stream; with the runtime's default of 4 hardware queues streams share a queue and
    // a 0.5 s scoring launch of one context stalls the small kernels of another (must be set before HIP initialises)
    setenv("GPU_MAX_HW_QUEUES", "16", 0);
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) {
        fprintf(stderr,
                "[ndgpu] FATAL: no HIP device visible (hipGetDeviceCount: %s). This library has no CPU fallback.\n",
                hipGetErrorString(e));
        abort();
    }
    const char *env = getenv("NDGPU_DEVICE");
    s_->device = env ? atoi(env) : 0;
    if (s_->device >= n) s_->device = s_->device % n;
    HIP_CHECK(hipSetDevice(s_->device));
    // A host thread that waits for its stream sleeps instead of spinning: eight driver threads spinning in hipStreamSynchronize are
    // eight cores the host phases of the other contexts do not get -- half of a 16-CPU container (NDGPU_SPIN_SYNC=1: the runtime's default)
    if (!getenv("NDGPU_SPIN_SYNC")) (void)hipSetDeviceFlags(hipDeviceScheduleBlockingSync);
    // Optional CU partition (NDGPU_RESERVED_CUS=n, default off): the first n compute units are kept for the scoring
    // launches of the small sub-batches that hold the longest seeds (lat_stream), every other kernel of every context
    // runs on the rest.  Measured on config 2: the long chains gain nothing (their 3.5 us per column is the chain
    // itself, not interference: 691 ms alone vs 821 ms with 8 contexts resident), so it stays off.
    {
        hipDeviceProp_t prop;
        HIP_CHECK(hipGetDeviceProperties(&prop, s_->device));
        const int n_cu = prop.multiProcessorCount;
        int reserve = 0;
        if (const char *e = getenv("NDGPU_RESERVED_CUS")) reserve = atoi(e);
        if (reserve < 0 || reserve * 2 > n_cu) reserve = 0;
        s_->reserved_cus = reserve;
        if (reserve) {
            const uint32_t words = (uint32_t)((n_cu + 31) / 32);
            std::vector<uint32_t> rest(words, 0), res(words, 0);
            for (int c = 0; c < n_cu; c++) (c < reserve ? res : rest)[c >> 5] |= 1u << (c & 31);
            HIP_CHECK(hipExtStreamCreateWithCUMask(&s_->stream, words, rest.data()));
            HIP_CHECK(hipExtStreamCreateWithCUMask(&s_->lat_stream, words, res.data()));
            HIP_CHECK(hipEventCreateWithFlags(&s_->ev_lat0, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&s_->ev_lat1, hipEventDisableTiming));
        } else {
            // contexts 0..2 receive the sub-batches with the longest seeds (capi.cpp deals sub-batch j to context j
            // in the first round): their kernels go first when the device is oversubscribed
            int least = 0, greatest = 0;
            HIP_CHECK(hipDeviceGetStreamPriorityRange(&least, &greatest));
            const int prio = (g_ctx_creating >= 0 && g_ctx_creating < 3 && !getenv("NDGPU_NO_STREAM_PRIO")) ? greatest : least;
            HIP_CHECK(hipStreamCreateWithPriority(&s_->stream, hipStreamNonBlocking, prio));
            HIP_CHECK(hipStreamCreateWithPriority(&s_->stream2, hipStreamNonBlocking, prio));
            HIP_CHECK(hipEventCreateWithFlags(&s_->ev_fork, hipEventDisableTiming));
            HIP_CHECK(hipEventCreateWithFlags(&s_->ev_join, hipEventDisableTiming));
        }
    }
#define NDGPU_NAME(T, x, place, level) s_->x.name = #x;
    NDGPU_BUFFERS(NDGPU_NAME)
#undef NDGPU_NAME
    const unsigned ev_flags = getenv("NDGPU_SPIN_SYNC") ? hipEventDefault : hipEventBlockingSync;  // (hipEventSynchronize sleeps, see above)
    for (auto &e : s_->evs) HIP_CHECK(hipEventCreateWithFlags(&e, ev_flags));
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) == hipSuccess && free_b > ((size_t)8 << 30))
        s_->trace_budget_bytes = std::min<size_t>(free_b / 24, (size_t)8 << 30);
    else s_->trace_budget_bytes = (size_t)2 << 30;
}

DeviceAligner::~DeviceAligner() { delete s_; }

static DeviceAligner *g_ctx[DeviceAligner::kMaxContexts] = {nullptr};
static std::mutex g_ctx_mu;

DeviceAligner &DeviceAligner::context(int i) {
    // intentionally leaked: no HIP calls at exit.  Contexts own a stream + buffer set each, so
    // batches driven from different host threads overlap on the device.
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    i = i < 0 ? 0 : i % kMaxContexts;
    if (!g_ctx[i]) {
        g_ctx_creating = i;
        g_ctx[i] = new DeviceAligner();
        g_ctx_creating = -1;
    }
    return *g_ctx[i];
}

DeviceAligner *DeviceAligner::peek(int i) {
    std::lock_guard<std::mutex> lock(g_ctx_mu);
    return g_ctx[i];
}

DeviceAligner &DeviceAligner::instance() { return context(0); }

RuntimeStats DeviceAligner::total_stats() {
    RuntimeStats t;
    for (int i = 0; i < kMaxContexts; i++) {
        DeviceAligner *cp = peek(i);
        if (!cp) continue;
        DeviceAligner &c = *cp;
        const RuntimeStats &s = c.s_->stats;
        t.tasks += s.tasks; t.wide_tasks += s.wide_tasks; t.cells += s.cells; t.d_steps += s.d_steps;
        t.trace_bits += s.trace_bits; t.trace_words += s.trace_words; t.lq_rounds += s.lq_rounds; t.lq_declined += s.lq_declined; t.lq_ms += s.lq_ms; t.columns += s.columns; t.pool_bases += s.pool_bases; t.seq_bases += s.seq_bases;
        t.max_band = s.max_band > t.max_band ? s.max_band : t.max_band;
        t.forward_launches += s.forward_launches; t.forward_ms += s.forward_ms; t.traceback_ms += s.traceback_ms;
        t.tags_ms += s.tags_ms; t.links_ms += s.links_ms; t.score_ms += s.score_ms; t.extract_ms += s.extract_ms;
        t.piles += s.piles; t.tags += s.tags; t.cells_msa += s.cells_msa; t.path_items += s.path_items;
        t.links += s.links; t.score_launches += s.score_launches; t.backtrack_ms += s.backtrack_ms;
        t.score_segments += s.score_segments; t.score_repairs += s.score_repairs; t.score_slow_piles += s.score_slow_piles;
        t.traceback_launches += s.traceback_launches; t.lq_launches += s.lq_launches; t.lq_columns += s.lq_columns;
        t.lq_aln_columns += s.lq_aln_columns; t.lq_bases += s.lq_bases; t.lq_out += s.lq_out; t.lq_jobs += s.lq_jobs; t.lq_repairs += s.lq_repairs;
        t.tb_tasks += s.tb_tasks; t.tb_walkers += s.tb_walkers; t.tb_fallbacks += s.tb_fallbacks;
        t.poa_jobs += s.poa_jobs; t.poa_declined += s.poa_declined; t.poa_rounds += s.poa_rounds; t.poa_launches += s.poa_launches;
        t.poa_cells += s.poa_cells; t.poa_ms += s.poa_ms;
        t.poa_resident_jobs += s.poa_resident_jobs; t.poa_resident_declined += s.poa_resident_declined;
        t.poa_graph_launches += s.poa_graph_launches; t.poa_graph_ms += s.poa_graph_ms;
        t.poa_h2d_bytes += s.poa_h2d_bytes; t.poa_d2h_bytes += s.poa_d2h_bytes;
        t.rank_jobs += s.rank_jobs; t.rank_tail += s.rank_tail; t.rank_launches += s.rank_launches; t.rank_ms += s.rank_ms;
        t.aln_batch_jobs += s.aln_batch_jobs; t.aln_batch_launches += s.aln_batch_launches; t.aln_batch_runs += s.aln_batch_runs;
        t.aln_batch_ms += s.aln_batch_ms;
        t.cns_jobs += s.cns_jobs; t.cns_declined += s.cns_declined; t.cns_launches += s.cns_launches; t.cns_regions += s.cns_regions;
        t.cns_ms += s.cns_ms; t.cns_d2h_bytes += s.cns_d2h_bytes; t.walk_d2h_bytes += s.walk_d2h_bytes;
        t.cnsw_hifi_jobs += s.cnsw_hifi_jobs; t.cnsw_hifi_declined += s.cnsw_hifi_declined; t.cnsw_hifi_regions += s.cnsw_hifi_regions;
        t.cnsw_fast_jobs += s.cnsw_fast_jobs; t.cnsw_fast_declined += s.cnsw_fast_declined; t.cnsw_launches += s.cnsw_launches;
        t.cnsw_ms += s.cnsw_ms; t.cnsw_d2h_bytes += s.cnsw_d2h_bytes;
        t.phase_piles += s.phase_piles; t.phase_regions += s.phase_regions; t.phase_pass2 += s.phase_pass2; t.phase_tail += s.phase_tail; t.phase_lower += s.phase_lower;
        for (int k = 0; k < 4; k++) t.phase_kind[k] += s.phase_kind[k];
        for (int k = 0; k < 5; k++) t.phase_declined[k] += s.phase_declined[k];
        t.phase_launches += s.phase_launches; t.phase_ms += s.phase_ms;
        t.phase_d2h_records += s.phase_d2h_records; t.phase_d2h_strings += s.phase_d2h_strings;
        t.splice_jobs += s.splice_jobs; t.splice_declined += s.splice_declined; t.splice_launches += s.splice_launches;
        t.splice_h2d_bytes += s.splice_h2d_bytes; t.splice_d2h_bytes += s.splice_d2h_bytes; t.splice_trimmed += s.splice_trimmed;
        t.splice_ms += s.splice_ms;
    }
    t.allocs = g_alloc_calls.load(), t.alloc_ms = (double)g_alloc_ns.load() * 1e-6;
    t.level_allocs = g_level_calls.load(), t.level_ms = (double)g_level_ns.load() * 1e-6;
    return t;
}

void DeviceAligner::reset_all_stats() {
    g_alloc_calls = 0, g_alloc_ns = 0, g_level_calls = 0, g_level_ns = 0;
    for (int i = 0; i < kMaxContexts; i++)
        if (DeviceAligner *c = peek(i)) c->reset_stats();
}

uint32_t *DeviceAligner::upload_db(const uint32_t *pool_words, size_t n_words, int device) {
    HIP_CHECK(hipSetDevice(device));
    uint32_t *d = nullptr;
    const hipError_t e = hipMalloc((void **)&d, (n_words + kPoolPadWords) * sizeof(uint32_t));
    if (e == hipErrorOutOfMemory) {
        (void)hipGetLastError();
        return nullptr;
    }
    HIP_CHECK(e);
    if (g_debug_alloc) fprintf(stderr, "[ndgpu alloc] db_pool %p .. %p\n", (void *)d, (void *)(d + n_words + kPoolPadWords));
    HIP_CHECK(hipMemcpy(d, pool_words, n_words * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIP_CHECK(hipMemset(d + n_words, 0, kPoolPadWords * sizeof(uint32_t)));
    return d;
}

void DeviceAligner::free_db(uint32_t *dev_pool) {
    if (!dev_pool) return;
    (void)hipDeviceSynchronize();
    (void)hipFree(dev_pool);
}

void DeviceAligner::use_db(const uint32_t *dev_pool) { s_->db_pool = dev_pool; }
int DeviceAligner::device() const { return s_->device; }

void DeviceAligner::release_memory() {
    State &S = *s_;
    std::lock_guard<std::mutex> lock(S.mu);
    (void)hipSetDevice(S.device);
    (void)hipStreamSynchronize(S.stream);
    if (S.stream2) (void)hipStreamSynchronize(S.stream2);
    (void)hipGetLastError();
    S.pending.clear();
    S.up_used = S.down_used = 0;
#define NDGPU_REL(T, x, place, level) S.x.release();
    NDGPU_BUFFERS(NDGPU_REL)
#undef NDGPU_REL
}

// After a batch call, with no kernel in flight: every context brings its buffers up to the sizes the largest sub-batch any context
// met has asked for, so that the next call -- whichever context then meets that sub-batch -- allocates nothing in the middle of
// a step.  (A context that is out of device memory keeps what it has.)
void DeviceAligner::level_buffers(int drivers) {
    struct Mark { Mark() { g_leveling++; } ~Mark() { g_leveling--; } } mark;
    for (int c = 0; c < drivers && c < kMaxContexts; c++) {
        DeviceAligner *d = peek(c);
        if (!d) continue;
        State &S = *d->s_;
        // a context with a batch open (another caller's thread) keeps its main-phase buffers alive between run_main and end_batch:
        // growing them here would free live device state.  It is skipped, like release_memory_if_idle skips it.
        std::unique_lock<State::OrderedLock> batch(S.batch_mu, std::try_to_lock);
        if (!batch.owns_lock()) continue;
        std::lock_guard<std::mutex> lock(S.mu);
        (void)hipSetDevice(S.device);
        size_t free_b = 0, total_b = 0;
        if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
        // (what the memory plan keeps free stays free: headroom + the caller's reservation for its other stage)
        long long budget = (long long)free_b - (long long)((size_t)10 << 30) - (long long)g_reserved_bytes.load();
        auto lvl = [&](auto &buf, bool device) {
            const size_t esz = sizeof(*buf.p);
            const size_t want = high_water(buf.name) / esz;
            if (want <= buf.cap) return;
            const long long growth = (long long)((want + want / 4 + 1024 - buf.cap) * esz);
            if (device) {
                if (growth > budget) return;
                budget -= growth;
            }
            buf.reserve(want);  // (while the device is idle: up to what any context has asked of the buffer of this name)
        };
        try {
#define NDGPU_LVL(T, x, place, level) \
    if (BufLevel::level == BufLevel::levelled) lvl(S.x, BufPlace::place == BufPlace::device);
            NDGPU_BUFFERS(NDGPU_LVL)
#undef NDGPU_LVL
        } catch (const DeviceOom &) {
        }
    }
}

void DeviceAligner::forget_sizes() { clear_high_water(); }

bool DeviceAligner::release_memory_if_idle() {
    if (!s_->batch_mu.try_lock()) return false;
    release_memory();
    s_->batch_mu.unlock();
    return true;
}

// How much of the device the consensus contexts may use, decided at the start of every batch call from what is free NOW
// (the overlap library's cache, the read DB and everything else stay where they are) plus what the contexts already
// hold: per context a trace budget (the forward / traceback chunk size) and a budget of alignment columns per sub-batch
// (~40 bytes of tags, column indexes, link tables and cell tables per column, growth slack included).
void DeviceAligner::reserve_device_memory(uint64_t bytes) { g_reserved_bytes = bytes; }

void DeviceAligner::plan_memory(int drivers, uint64_t *tag_budget) {
    size_t free_b = 0, total_b = 0;
    const int dev = context(0).device();
    (void)hipSetDevice(dev);
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) return;
    const long long held = g_dev_bytes.load();
    long long avail = (long long)free_b + held - (long long)((size_t)10 << 30)   // headroom: runtime, pinned staging
                      - (long long)g_reserved_bytes.load();                      // what the caller's other stage will need again
    if (const char *e = getenv("NDGPU_DEVICE_BUDGET_GB")) avail = std::min<long long>(avail, (long long)(atof(e) * (double)(1ull << 30)));
    if (avail < ((long long)4 << 30)) avail = (long long)4 << 30;
    const long long per_ctx = avail / std::max(1, drivers);
    const size_t trace = (size_t)std::min<long long>((long long)8 << 30, std::max<long long>(per_ctx / 5, (long long)256 << 20));
    const long long cols = (per_ctx - (long long)trace - ((long long)1 << 30)) / 40;
    *tag_budget = (uint64_t)std::min<long long>(900000000ll, std::max<long long>(20000000ll, cols));
    for (int i = 0; i < drivers && i < kMaxContexts; i++) context(i).s_->trace_budget_bytes = trace;
    if (trace_on())
        fprintf(stderr, "[ndgpu trace] memory plan: %.1f GB free + %.1f GB held by the contexts -> %d contexts x (%.1f GB trace + %llu M columns)\n",
                free_b / 1073741824.0, held / 1073741824.0, drivers, trace / 1073741824.0, (unsigned long long)(*tag_budget / 1000000));
}

void *DeviceAligner::stream() const { return s_->stream; }
RuntimeStats DeviceAligner::stats() const { return s_->stats; }
void DeviceAligner::reset_stats() { s_->stats = RuntimeStats(); }

static inline uint64_t wall_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}


static void limits_for(int total, int hq, int *max_d, int *band) {
    // lib/align.c:567-568,575-576 -- double arithmetic on the host, exactly as the reference
    if (hq) {
        *max_d = (int)((total > 1000 ? 0.1 : 0.5) * total);
        *band = (int)((total > 1000 ? 0.03 : 0.3) * total);
    } else {
        *max_d = (int)(0.4 * total);
        *band = (int)((total > 5000 ? 0.1 : 1) * total);
    }
}

// Test hooks and A/B knobs, a struct per phase, each read once per process at the first call of its phase.
template <typename H>
static const H &hooks_of() { static const H h; return h; }

// ---- the traceback in segments (ond_kernels.hip: tb_chase / tb_walk / tb_stitch) ----
// NDGPU_K8_SEG = rows per walker (a power of two; 0: the one-lane kernel everywhere), NDGPU_K8_WARM = rows a walker walks before the rows
// it owns, NDGPU_K8_MINLEN = a launch takes the segmented path when its longest pair has at least that many bases (q + t).  Test hooks
// and A/B knobs; the defaults are what the bench was measured with.
struct TbConfig {
    int cshift = 8, warm = 32;
    bool on = true;
    uint32_t minlen = 8192;
    TbConfig() {
        if (const char *e = getenv("NDGPU_K8_SEG")) {
            const int c = atoi(e);
            on = c >= 4;
            cshift = 2;
            while ((2 << cshift) <= c) cshift++;
        }
        if (const char *e = getenv("NDGPU_K8_WARM")) warm = atoi(e);
        if (warm < 1) warm = 1;
        if (warm > (1 << cshift)) warm = 1 << cshift;
        if (const char *e = getenv("NDGPU_K8_MINLEN")) minlen = (uint32_t)atoll(e);
    }
};
struct MainHooks {  // the main phase (run_main)
    uint32_t k10_seg_len = 1024;    // NDGPU_K10_SEG: columns of a K10 segment (the last one of a pile takes the remainder)
    uint32_t k10_warm = 128;        // NDGPU_K10_WARM: warm-up columns of a speculative segment (< seg_len)
    int32_t k10_guard = 1 << 30;    // NDGPU_K10_GUARD: raw scores beyond it send the pile to the int64 kernel
    // NDGPU_K10_FORCE = large (every pile through the large tables) | slow (every pile through the int64 HBM-resident kernel) |
    // seq (one segment per pile: no speculation) | repair (every second segment is scored again by the stitch kernel as if its
    // check had failed)
    bool k10_large = false, k10_slow = false;
    uint32_t k10_force_repair = 0;
    bool k7_order = !getenv("NDGPU_K7_NO_ORDER");                 // NDGPU_K7_NO_ORDER: K7 in table order, not longest first
    bool k8_order = getenv("NDGPU_K8_ORDER") != nullptr;          // NDGPU_K8_ORDER: K8a in K7's order (see align_main)
    bool k9_full = getenv("NDGPU_K9_FULL") != nullptr;            // NDGPU_K9_FULL: skip the small-capacity first attempt of K9
    bool k9_force_retry = getenv("NDGPU_K9_FORCE_RETRY") != nullptr;  // NDGPU_K9_FORCE_RETRY: take the overflow path behind attempt 0
    bool k9_digest = getenv("NDGPU_K9_DIGEST") != nullptr && atoi(getenv("NDGPU_K9_DIGEST")) != 0;  // NDGPU_K9_DIGEST: see k9_digest_trace
    MainHooks() {
        if (const char *e = getenv("NDGPU_K10_SEG")) k10_seg_len = (uint32_t)std::max(16, atoi(e));
        if (const char *e = getenv("NDGPU_K10_WARM")) k10_warm = (uint32_t)std::max(1, atoi(e));
        if (const char *e = getenv("NDGPU_K10_GUARD")) k10_guard = atoi(e);
        if (const char *e = getenv("NDGPU_K10_FORCE")) {
            k10_large = !strcmp(e, "large"), k10_slow = !strcmp(e, "slow");
            if (!strcmp(e, "seq")) k10_seg_len = 0x7fffffffu;
            if (!strcmp(e, "repair")) k10_force_repair = 2;
        }
        if (k10_warm >= k10_seg_len) k10_warm = k10_seg_len - 1;
    }
};
struct LqHooks {
    // NDGPU_K12_MAX_COLUMNS: a pile whose linked pseudo-seed is longer is left to the host path.  (12,000 until round 4, when K12b was one
    // wavefront per pile; scored job by job the chain is as long as a job, and the bound is what the packed records can address.)
    uint64_t max_cols = env_u64("NDGPU_K12_MAX_COLUMNS", 400000);
    // NDGPU_K12_JOB_COLUMNS: columns of a K12a job (a pile of 3,000 columns is ~15 wavefronts' worth of link building; 1 = every region a job)
    uint64_t job_cols = env_u64("NDGPU_K12_JOB_COLUMNS", 192);
    // NDGPU_K12_WARM: columns a K12b job starts before its own first one (speculative start, checked by the stitch)
    uint32_t warm = (uint32_t)std::max(1, getenv("NDGPU_K12_WARM") ? atoi(getenv("NDGPU_K12_WARM")) : 64);
    // NDGPU_K12_FORCE=repair: every second job is scored again by the stitch kernel as if its boundary check had failed
    uint32_t force_repair = env_is("NDGPU_K12_FORCE", "repair") ? 2u : 0u;
};
struct PoaHooks {
    bool budget_set = getenv("NDGPU_POA_BUDGET") != nullptr;  // NDGPU_POA_BUDGET: the cell budget of a launch, in place of a sixth
    uint64_t budget = env_u64("NDGPU_POA_BUDGET", 0);         // of the trace budget's bytes (0: every problem is declined)
    int form = env_is("NDGPU_POA_FORM", "wave") ? 1 : env_is("NDGPU_POA_FORM", "group") ? 2 : 0;  // the kernel form every job takes
    uint32_t group_min = (uint32_t)env_u64("NDGPU_POA_GROUP_MIN", kPoaGroupMinLen);  // the query length the workgroup form takes over from
    bool resident = env_is("NDGPU_POA_RESIDENT", "1");  // the graphs live on the device (K19); unset: K13's rounds with the graphs on the host
};
struct ExtractHooks {
    // NDGPU_EXTRACT_POOL=bytes: the first guess of K11's string pool (extract_into_pool) -- a small one makes the first call of a
    // process retake the pool, a path no fixture reaches otherwise
    bool pool_set = getenv("NDGPU_EXTRACT_POOL") != nullptr;
    size_t pool = (size_t)env_u64("NDGPU_EXTRACT_POOL", 0);
};
static inline uint32_t tb_ck_slots(int max_d) { return max_d > 0 ? (uint32_t)(max_d - 1) >> hooks_of<TbConfig>().cshift : 0u; }
// device bytes a task adds to its launch when the launch is walked in segments
static inline uint64_t tb_bytes(int max_d) {
    if (!hooks_of<TbConfig>().on) return 0;
    const uint64_t k = tb_ck_slots(max_d);
    return k * (kCkptCells * sizeof(uint32_t) + sizeof(uint2)) + (k + 1) * (sizeof(TbSeg) + sizeof(TbSegOut));
}
// tasks [a, b) of one launch: their checkpoint / walker slots (AlnTask::mink_off, seg_off); false: the launch keeps the one-lane kernel
static bool tb_assign(AlnTask *tasks, size_t a, size_t b, uint64_t *ck_slots, uint64_t *seg_slots) {
    const TbConfig &c = hooks_of<TbConfig>();
    *ck_slots = *seg_slots = 0;
    if (!c.on) return false;
    uint32_t longest = 0;
    for (size_t i = a; i < b; i++) {
        if ((uint32_t)tasks[i].q_len >= (1u << 24)) return false;  // (a checkpoint cell holds x in 24 bits)
        longest = std::max(longest, (uint32_t)tasks[i].q_len + (uint32_t)tasks[i].t_len);
    }
    if (longest < c.minlen) return false;
    uint64_t ck = 0, sg = 0;
    for (size_t i = a; i < b; i++) {
        const uint32_t k = tb_ck_slots(tasks[i].max_d);
        tasks[i].mink_off = ck;
        tasks[i].seg_off = (uint32_t)sg;
        ck += k;
        sg += k + 1;
    }
    if (sg >= (1ull << 31)) return false;
    *ck_slots = ck;
    *seg_slots = sg;
    return true;
}

// ---- the align phase: what run_chunk, run_lq and run_main do alike between "my tasks are built" and "the AlnOut records are here" ----
// The fields of a task that follow from its lengths (q_len and t_len are set): the reference's limits, the register path's rows, its
// region of the ops buffer -- and the counter of operand bases.  q_off / t_off and pool_bases differ by caller and stay there.
static void task_limits(AlnTask &t, int hq, uint64_t &ops_words, RuntimeStats &stats) {
    int md, bd;
    limits_for(t.q_len + t.t_len, hq, &md, &bd);
    t.max_d = md;
    t.band = bd;
    t.row_words = kFastRowWords;
    t.ops_off = ops_words;
    t.ops_cap = (uint32_t)(t.q_len + t.t_len);
    ops_words += (uint64_t)(t.ops_cap + 15) / 16 + 1;
    stats.seq_bases += (uint64_t)t.q_len + (uint64_t)t.t_len;
}
// device bytes a task adds to its launch: its trace rows and its share of the traceback in segments.  The one rule chunks are cut by.
static inline uint64_t task_trace_bytes(int max_d) { return (uint64_t)max_d * (kFastRowWords * 8) + tb_bytes(max_d); }

// Cuts tasks [0, nt) into launches bounded by the trace budget (a task on its own always fits), gives every task its trace rows and its
// checkpoint / walker slots within its launch, and reserves d_trace and the traceback's four buffers for the largest launch.
std::vector<AlignChunk> DeviceAligner::State::plan_chunks(AlnTask *t, size_t nt) {
    std::vector<AlignChunk> chunks;
    uint64_t max_tw = 0, max_ck = 0, max_sg = 0;
    for (size_t a = 0; a < nt;) {
        uint64_t tw = 0, bytes = 0;
        size_t b = a;
        for (; b < nt; b++) {
            const uint64_t need = task_trace_bytes(t[b].max_d);
            if (b > a && bytes + need > trace_budget_bytes) break;
            t[b].trace_off = tw;
            tw += (uint64_t)t[b].max_d * kFastRowWords;
            bytes += need;
        }
        uint64_t ck = 0, sg = 0;
        const bool seg = tb_assign(t, a, b, &ck, &sg);
        max_tw = std::max(max_tw, tw);
        max_ck = std::max(max_ck, ck);
        max_sg = std::max(max_sg, sg);
        chunks.push_back(AlignChunk{a, b, seg, sg});
        a = b;
    }
    d_trace.reserve(max_tw + kTracePadWords);
    if (max_sg) {
        d_ck_cells.reserve(max_ck * kCkptCells + 1);
        d_ck_hdr.reserve(max_ck + 1);
        d_tbseg.reserve(max_sg);
        d_tbout.reserve(max_sg);
    }
    return chunks;
}

// K7 + K8a of one chunk on the context's stream.  order / tb_order: device lists of the chunk's task ids (nullptr: table order).
// ev_mid is recorded between the two kernels, ev_end (if given) behind the traceback; who names the caller in the debug lines.
void DeviceAligner::State::launch_chunk(const AlignChunk &c, const int32_t *order, const int32_t *tb_order, hipEvent_t ev_mid,
                                        hipEvent_t ev_end, const char *who) {
    const AlnTask *tk = d_tasks.p + c.begin;
    AlnOut *out = d_outs.p + c.begin;
    const int n = (int)(c.end - c.begin);
    const TbArgs tb{d_ck_cells.p, d_ck_hdr.p, d_tbseg.p, d_tbout.p, (int)c.slots, hooks_of<TbConfig>().cshift, hooks_of<TbConfig>().warm};
    if (c.seg) launch_ond_forward_ckpt(tk, out, d_pool.p, db_pool, d_trace.p, d_ops.p, tb, n, stream, order);
    else launch_ond_forward(tk, out, d_pool.p, db_pool, d_trace.p, n, stream, order);
    HIP_CHECK(hipEventRecord(ev_mid, stream));
    if (who) NDGPU_DBG(stream, "%s: traceback", who);
    if (c.seg) launch_ond_traceback_seg(tk, out, d_pool.p, db_pool, d_trace.p, d_ops.p, tb, n, stream);
    else launch_ond_traceback(tk, out, d_pool.p, db_pool, d_trace.p, nullptr, d_ops.p, nullptr, n, stream, tb_order);
    if (ev_end) HIP_CHECK(hipEventRecord(ev_end, stream));
}

// The counters the AlnOut records h_outs[0, nt) feed; wide (if given) collects the tasks whose live band left the register path.
void DeviceAligner::State::tally_outs(size_t nt, std::vector<int32_t> *wide) {
    for (size_t i = 0; i < nt; i++) {
        const AlnOut &o = h_outs.p[i];
        stats.cells += (uint64_t)o.cells;
        stats.d_steps += (uint64_t)o.d_steps;
        stats.trace_words += (uint64_t)o.trace_end;
        if (o.fin_idx & kTbSeen) {
            stats.tb_tasks++;
            stats.tb_walkers += (uint64_t)(o.d_final > 0 ? (o.d_final - 1) >> hooks_of<TbConfig>().cshift : 0) + 1;
            if (o.fin_idx & kTbRefused) stats.tb_fallbacks++;
        }
        if ((uint32_t)o.max_band > stats.max_band) stats.max_band = (uint32_t)o.max_band;
        if (wide && o.status == ST_NEED_WIDE) wide->push_back((int32_t)i);
        if (o.status == ST_ALIGNED) {  // (K8a's output: 2-bit column kinds -- the term bench.py's roofline prices it with)
            stats.trace_bits += (uint64_t)o.cells;
            stats.columns += (uint64_t)o.n_cols;
        }
    }
}

// How many of jobs[0, n) make the next chunk: as many as fit the trace budget -- one chunk of plan_chunks, which chunk_front relies on.
// NDGPU_ALIGN_CHUNK_JOBS (test hook, read once): at most that many jobs a chunk.
static size_t next_chunk(AlnJob *const *jobs, size_t n, uint64_t trace_budget_bytes) {
    static const size_t max_jobs = getenv("NDGPU_ALIGN_CHUNK_JOBS") ? (size_t)std::max(1ll, atoll(getenv("NDGPU_ALIGN_CHUNK_JOBS"))) : ~(size_t)0;
    size_t take = 0;
    uint64_t bytes = 0;
    while (take < n && take < max_jobs) {
        const AlnJob &j = *jobs[take];
        int md, bd;
        limits_for(j.q_len + j.t_len, j.hq, &md, &bd);
        const uint64_t b = task_trace_bytes(md);
        if (take && bytes + b > trace_budget_bytes) break;
        bytes += b;
        take++;
    }
    return take;
}

void DeviceAligner::align_batch(AlnJob **jobs, size_t n) {
    if (n == 0) return;
    const State::Phase phase(*s_);
    for (size_t done = 0; done < n;) {
        const size_t take = next_chunk(jobs + done, n - done, s_->trace_budget_bytes);
        run_chunk(jobs + done, take);
        done += take;
    }
}

void DeviceAligner::align_batch_runs(AlnJob **jobs, size_t n, AlnRunsResult *res, std::vector<uint32_t> &runs) {
    runs.clear();
    if (n == 0) return;
    const State::Phase phase(*s_);
    for (size_t done = 0; done < n;) {
        const size_t take = next_chunk(jobs + done, n - done, s_->trace_budget_bytes);
        run_chunk_runs(jobs + done, take, res + done, runs);
        done += take;
    }
}

namespace {
template <typename F>
void par_ranges(size_t n, int base_threads, F f) {  // f(begin, end) over contiguous ranges: a chunk's jobs, packed / decoded
    host_ranges(n, base_threads <= 1 || n < 4096, base_threads, (n + 2047) / 2048, f);
}

}  // namespace

void DeviceAligner::set_host_threads(int n) { s_->host_threads = n < 1 ? 1 : n; }

// The front of a chunk, whatever becomes of its column streams: tasks laid out, sequences packed and uploaded, K7 / K8a launched, the
// AlnOut records on the host (h_outs), the wide-band tasks run again.  ops_to_host: the ops come down with the records (h_ops).
// bad[i]: job i has a byte the packer rejects; dev_ns: wall time from the first upload to the last record.  Returns the chunk's ops words.
uint64_t DeviceAligner::chunk_front(AlnJob **jobs, size_t n, std::vector<uint8_t> &bad, bool ops_to_host, uint64_t *dev_ns) {
    State &S = *s_;
    std::vector<uint32_t> &pool = S.pool;
    std::vector<AlnTask> &tasks = S.tasks;
    tasks.assign(n, AlnTask());
    bad.assign(n, 0);
    // pass 1 (serial, O(1) per job): offsets of every per-task region
    std::vector<uint64_t> qw(n + 1), tw(n + 1);
    uint64_t ops_words = 0, pool_words = 0;
    for (size_t i = 0; i < n; i++) {
        const AlnJob &j = *jobs[i];
        AlnTask &t = tasks[i];
        t.q_len = j.q_len;
        t.t_len = j.t_len;
        qw[i] = pool_words;
        if (j.q_dev < 0) pool_words += ((uint64_t)j.q_len + 15) / 16;
        tw[i] = pool_words;
        if (j.t_dev < 0) pool_words += ((uint64_t)j.t_len + 15) / 16;
        task_limits(t, j.hq, ops_words, S.stats);
        S.stats.pool_bases += (j.q_dev < 0 ? (uint64_t)j.q_len : 0) + (j.t_dev < 0 ? (uint64_t)j.t_len : 0);
    }
    pool.assign(pool_words, 0);
    // pass 2 (parallel): pack the sequences
    par_ranges(n, S.host_threads, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            AlnJob &j = *jobs[i];
            AlnTask &t = tasks[i];
            if (ops_to_host) {
                j.status = ALN_NONE;
                j.ops.clear();
                j.q_used = j.t_used = 0;
            }
            if (j.q_dev >= 0) t.q_off = (uint64_t)j.q_dev | kOffDb;
            else {
                t.q_off = qw[i] * 16;
                if (!pack_into(pool.data() + qw[i], j.q, (size_t)j.q_len)) bad[i] = 1;
            }
            if (j.t_dev >= 0) t.t_off = (uint64_t)j.t_dev | kOffDb;
            else {
                t.t_off = tw[i] * 16;
                if (!pack_into(pool.data() + tw[i], j.t, (size_t)j.t_len)) bad[i] = 1;
            }
            if (bad[i]) t.max_d = 0;
        }
    });
    pool.insert(pool.end(), kPoolPadWords, 0u);  // the kernels fetch up to five words from a sequence's last base on

    S.d_pool.reserve(pool.size());
    S.d_tasks.reserve(n);
    S.d_outs.reserve(n);
    const std::vector<AlignChunk> chunks = S.plan_chunks(tasks.data(), n);
    assert(chunks.size() == 1);  // next_chunk cut the jobs by the same rule (a task marked bad only shrinks the chunk)
    S.d_ops.reserve(ops_words + 2);
    if (ops_to_host) S.h_ops.reserve(ops_words + 2);
    S.h_outs.reserve(n);

    hipStream_t st = S.stream;
    const uint64_t tc1 = wall_ns();
    S.h2d(S.d_pool.p, pool.data(), pool.size() * sizeof(uint32_t), st);
    S.h2d(S.d_tasks.p, tasks.data(), n * sizeof(AlnTask), st);
    S.mark(State::kEvFrontK7, st);
    NDGPU_DBG(st, "chunk: forward %zu tasks", n);
    S.launch_chunk(chunks[0], nullptr, nullptr, S.evs[State::kEvFrontK8a], nullptr, "chunk");
    NDGPU_DBG(st, "chunk: done");
    HIP_CHECK(hipMemcpyAsync(S.h_outs.p, S.d_outs.p, n * sizeof(AlnOut), hipMemcpyDeviceToHost, st));
    if (ops_to_host) HIP_CHECK(hipMemcpyAsync(S.h_ops.p, S.d_ops.p, ops_words * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    S.sync_drain(st);
    HIP_CHECK(hipGetLastError());
    S.stats.forward_ms += S.ms(State::kEvFrontK7, State::kEvFrontK8a);  // (this path brackets K7 alone: its K8a is in neither traceback_ms nor traceback_launches)
    S.stats.forward_launches++;
    S.stats.tasks += n;

    // rare: live band wider than the LDS fast path -> rerun those with V in HBM
    std::vector<int32_t> wide;
    for (size_t i = 0; i < n; i++)
        if (S.h_outs.p[i].status == ST_NEED_WIDE) wide.push_back((int32_t)i);
    if (!wide.empty()) S.run_wide(ops_to_host, wide);
    *dev_ns = wall_ns() - tc1;

    S.tally_outs(n, nullptr);  // (after run_wide: the wide tasks count with what the wide kernels reported)
    if (std::find(bad.begin(), bad.end(), 1) != bad.end()) {
        static bool warned = false;
        if (!warned) {
            fprintf(stderr, "[ndgpu] sequence with bytes outside [ACGT]: alignment skipped\n");
            warned = true;
        }
    }
    return ops_words;
}

// Columns [first_col, first_col + n) of a task's 2-bit column kinds, a byte a column.
static void unpack_cols(const uint32_t *W, uint32_t first_col, uint32_t n, std::vector<uint8_t> &out) {
    out.resize(n);
    for (uint32_t c = 0, cc = first_col; c < n; c++, cc++) out[c] = (uint8_t)((W[cc >> 4] >> ((cc & 15u) * 2u)) & 3u);
}

// The tail of run_align, the LQ host path and align(): the column kinds come down with the records and are unpacked, a byte a column.
void DeviceAligner::run_chunk(AlnJob **jobs, size_t n) {
    State &S = *s_;
    const uint64_t tc0 = wall_ns();
    uint64_t dev_ns = 0;
    std::vector<uint8_t> bad;
    chunk_front(jobs, n, bad, true, &dev_ns);
    const std::vector<AlnTask> &tasks = S.tasks;
    const uint64_t tc2 = wall_ns();
    par_ranges(n, S.host_threads, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            AlnJob &j = *jobs[i];
            const AlnOut &o = S.h_outs.p[i];
            const AlnTask &t = tasks[i];
            if (bad[i]) continue;
            if (o.status == ST_ALIGNED) {
                j.status = ALN_OK;
                j.q_used = o.x_final;
                j.t_used = o.y_final;
                unpack_cols(S.h_ops.p + t.ops_off, t.ops_cap - (uint32_t)o.n_cols, (uint32_t)o.n_cols, j.ops);
            } else if (o.status == ST_GAP_ABORT) {
                j.status = ALN_GAP_ABORT;
                j.q_used = o.x_final;
                j.t_used = o.y_final;
                unpack_cols(S.h_ops.p + t.ops_off, t.ops_cap - 2, 2, j.ops);  // the reference reports aln_len = 2: the last two alignment columns
            } else {
                j.status = ALN_NONE;
            }
        }
    });
    // (host packing = the front less its device round trip)
    g_prof.c_pack += tc2 - tc0 - dev_ns, g_prof.c_dev += dev_ns, g_prof.c_decode += wall_ns() - tc2, g_prof.c_jobs += n;
}

// The batched entry's tail: the column streams stay in HBM.  K15 counts every task's runs, the summaries come down (they are the
// caller's anyway, and the host has to know the total to size the runs' buffer exactly -- so the exclusive scan of n_runs is done
// here, on the n numbers at hand, and goes up as n offsets: a device scan would save that upload and nothing else, the
// synchronisation in between stays), K15 emits, and exactly the runs come down behind what earlier chunks of the call left in `runs`.
void DeviceAligner::run_chunk_runs(AlnJob **jobs, size_t n, AlnRunsResult *res, std::vector<uint32_t> &runs) {
    State &S = *s_;
    std::vector<uint8_t> bad;
    uint64_t dev_ns = 0;
    chunk_front(jobs, n, bad, false, &dev_ns);
    hipStream_t st = S.stream;
    const bool any_bad = std::find(bad.begin(), bad.end(), 1) != bad.end();
    if (any_bad) {
        std::vector<uint32_t> bits((n + 31) / 32, 0u);
        for (size_t i = 0; i < n; i++)
            if (bad[i]) bits[i >> 5] |= 1u << (i & 31);
        S.d_run_skip.reserve(bits.size());
        S.h2d(S.d_run_skip.p, bits.data(), bits.size() * sizeof(uint32_t), st);
    }
    S.d_run_sums.reserve(n);
    std::vector<AlnRunSum> sums(n);
    S.mark(State::kEvTailBegin, st);
    NDGPU_DBG(st, "chunk: K15 count, %zu tasks", n);
    launch_aln_runs_count(S.d_tasks.p, S.d_outs.p, S.d_ops.p, any_bad ? S.d_run_skip.p : nullptr, S.d_run_sums.p, (int)n, st);
    HIP_CHECK(hipGetLastError());
    S.mark(State::kEvTailEnd, st);
    S.d2h(sums.data(), S.d_run_sums.p, n * sizeof(AlnRunSum), st);
    S.sync_drain(st);
    S.stats.aln_batch_ms += S.ms(State::kEvTailBegin, State::kEvTailEnd);

    std::vector<uint64_t> off(n);
    uint64_t total = 0;
    for (size_t i = 0; i < n; i++) {
        off[i] = total;
        total += sums[i].n_runs;
    }
    const size_t at = runs.size();
    runs.resize(at + total);
    if (total) {
        S.d_run_off.reserve(n);
        S.d_runs.reserve(total);
        S.h2d(S.d_run_off.p, off.data(), n * sizeof(uint64_t), st);
        S.mark(State::kEvTailBegin, st);
        NDGPU_DBG(st, "chunk: K15 emit, %llu runs", (unsigned long long)total);
        launch_aln_runs_emit(S.d_tasks.p, S.d_outs.p, S.d_ops.p, S.d_run_sums.p, S.d_run_off.p, S.d_runs.p, (int)n, st);
        HIP_CHECK(hipGetLastError());
        S.mark(State::kEvTailEnd, st);
        S.d2h(runs.data() + at, S.d_runs.p, total * sizeof(uint32_t), st);
        S.sync_drain(st);
        S.stats.aln_batch_ms += S.ms(State::kEvTailBegin, State::kEvTailEnd);
        S.stats.aln_batch_launches++;
    }
    S.stats.aln_batch_jobs += n;
    S.stats.aln_batch_runs += total;
    for (size_t i = 0; i < n; i++) {
        const AlnOut &o = S.h_outs.p[i];
        const AlnRunSum &u = sums[i];
        AlnRunsResult &r = res[i];
        r = AlnRunsResult();
        r.run_off = at + off[i];
        if (bad[i] || (o.status != ST_ALIGNED && o.status != ST_GAP_ABORT)) continue;
        r.status = o.status == ST_ALIGNED ? ALN_OK : ALN_GAP_ABORT;
        r.q_used = (uint32_t)o.x_final, r.t_used = (uint32_t)o.y_final;
        r.aln_len = u.aln_len, r.n_match = u.n_match, r.n_ins = u.n_ins, r.n_del = u.n_del, r.max_gap_run = u.max_gap_run;
        r.n_runs = u.n_runs;
    }
}

void DeviceAligner::State::run_wide(bool ops_to_host, const std::vector<int32_t> &ids) {  // (ops_to_host false: the main phase keeps ops in HBM)
    State &S = *this;
    // process in groups bounded by the trace budget; wide rows are band-cap sized
    size_t at = 0;
    DevBuf<uint64_t> &trace = S.d_wtrace;
    DevBuf<int32_t> &mink = S.d_wmink;
    while (at < ids.size()) {
        size_t take = 0;
        uint64_t tw = 0, mr = 0, vw = 0;
        uint32_t max_ring = 0;
        std::vector<AlnTask> patch;
        while (at + take < ids.size()) {
            AlnTask t = S.tasks[ids[at + take]];
            const uint32_t rw = (uint32_t)((t.band / 2 + 2 + 63) / 64);
            uint32_t ring = 256;
            while (ring < (uint32_t)t.band + 4) ring <<= 1;
            const uint64_t need = (uint64_t)t.max_d * rw * 8;
            if (take && (tw * 8 + need) > S.trace_budget_bytes) break;
            t.row_words = rw;
            t.trace_off = tw;
            t.mink_off = mr;
            t.v_off = vw;
            t.v_mask = ring - 1;
            tw += (uint64_t)t.max_d * rw;
            mr += (uint64_t)t.max_d;
            vw += ring;
            max_ring = std::max(max_ring, ring);
            patch.push_back(t);
            take++;
        }
        trace.reserve(tw + 2);
        mink.reserve(mr + 2);
        S.d_v.reserve(vw + 2);
        S.d_ids.reserve(take);
        S.d_wtasks.reserve(take);
        hipStream_t st = S.stream;
        // the group's records go up as ONE table in list order (the kernels of this path read it; the main table keeps the register
        // path's fields, which nobody reads again) and the whole span of results comes back in ONE copy: a task at a time was 2 x 8,307
        // blit kernels per step of the ultra-long read set
        int32_t lo = ids[at], hi = ids[at];
        for (size_t i = 0; i < take; i++) {
            S.tasks[ids[at + i]] = patch[i];
            lo = std::min(lo, ids[at + i]);
            hi = std::max(hi, ids[at + i]);
        }
        S.h2d(S.d_wtasks.p, patch.data(), take * sizeof(AlnTask), st);
        S.h2d(S.d_ids.p, ids.data() + at, take * sizeof(int32_t), st);
        launch_ond_forward_wide(S.d_tasks.p, S.d_outs.p, S.d_pool.p, S.db_pool, trace.p, mink.p, S.d_v.p, S.d_ids.p, (int)take, st, S.d_wtasks.p, max_ring);
        launch_ond_traceback(S.d_tasks.p, S.d_outs.p, S.d_pool.p, S.db_pool, trace.p, mink.p, S.d_ops.p, S.d_ids.p, (int)take, st, nullptr,
                             S.d_wtasks.p);
        HIP_CHECK(hipMemcpyAsync(S.h_outs.p + lo, S.d_outs.p + lo, (size_t)(hi - lo + 1) * sizeof(AlnOut), hipMemcpyDeviceToHost, st));
        S.sync_drain(st);
        for (size_t i = 0; i < take; i++) {
            const int32_t id = ids[at + i];
            const AlnTask &t = S.tasks[id];
            if (ops_to_host)
                HIP_CHECK(hipMemcpy(S.h_ops.p + t.ops_off, S.d_ops.p + t.ops_off,
                                    ((uint64_t)(t.ops_cap + 15) / 16 + 1) * sizeof(uint32_t), hipMemcpyDeviceToHost));
        }
        S.stats.wide_tasks += take;
        at += take;
    }
}

constexpr uint32_t kLenClasses = 16384;  // 64-base length classes of the longest-first launch order (length_order); the last one holds >= 1 Mb

// ---- low-quality-region rounds of a batch of piles on the device: K7 / K8a over every (row, region) alignment, then K12 (lq_links +
// lq_score: linked pseudo-seed, second MSA, DP, walk) -- the column streams stay in HBM, what comes back is each pile's walk string.
// A round the kernel declines (r->ok stays false) is left to the caller's host path.  run_lq (below) is the sequence of these steps:
//   layout_lq (a round at a time, its jobs cut by cut_lq_jobs of nd_lqplan.h) -> pack_lq_pool -> reserve_lq (buffers, align chunks) ->
//   launch_lq (uploads, K7 / K8a chunk by chunk, K12, downloads, the one synchronisation) -> tally_lq (events, verdicts, stats).

// One round: its pieces, tasks (one per piece with a job), sequence words (candidates once each, pseudo-seeds once per region), jobs
// and output regions, appended to the layout.  L.usable[r] stays 0 where the round is left to the host path.
void DeviceAligner::State::layout_lq_round(LqRound &R, size_t r, LqLayout &L) {
    R.ok = false;
    R.lqc.clear();
    LqPileDev &P = L.piles[r];
    memset(&P, 0, sizeof(P));
    const uint32_t nr = R.n_regions;
    if (nr == 0 || R.pieces.size() != (size_t)nr * kLqRoundRows) return;
    uint64_t link_len = 1, ins_cap = 0;
    for (uint32_t g = 0; g < nr; g++) link_len += (uint64_t)R.pieces[g].sl + 1;
    if (link_len > hooks_of<LqHooks>().max_cols) return;
    P.first_piece = (uint32_t)L.pieces.size(), P.n_regions = nr, P.factor = R.factor, P.qv_factor = R.qv_factor;
    std::vector<uint64_t> t_off(nr, ~0ull);  // word offset of every region's pseudo-seed, packed on first use
    std::vector<LqRegionLoad> load(nr);      // what cut_lq_jobs sizes the jobs' streams by
    for (uint32_t g = 0; g < nr; g++) load[g] = LqRegionLoad{R.pieces[g].sl, 0, 0, 0};
    for (size_t k = 0; k < R.pieces.size(); k++) {
        const LqRound::Piece &pc = R.pieces[k];
        const uint32_t g = (uint32_t)(k % nr);
        LqPieceDev d{-1, pc.sl};
        if (pc.job >= 0) {
            const AlnJob &j = (*R.jobs)[(size_t)pc.job];
            AlnTask t;
            memset(&t, 0, sizeof(t));
            t.q_len = j.q_len, t.t_len = j.t_len;
            L.srcs.push_back(LqSrc{j.q_words, j.q, (uint32_t)j.q_len, L.pool_words});
            t.q_off = L.pool_words * 16;
            L.pool_words += ((uint64_t)j.q_len + 15) / 16;
            if (t_off[g] == ~0ull) {
                t_off[g] = L.pool_words;
                L.srcs.push_back(LqSrc{nullptr, j.t, (uint32_t)j.t_len, L.pool_words});
                L.pool_words += ((uint64_t)j.t_len + 15) / 16;
            }
            t.t_off = t_off[g] * 16;
            task_limits(t, j.hq, L.ops_words, stats);
            ins_cap += (uint64_t)j.q_len;
            load[g].q_bases += (uint64_t)j.q_len, load[g].qt_bases += (uint64_t)j.q_len + (uint64_t)j.t_len;
            d.task = (int32_t)tasks.size();
            tasks.push_back(t);
            stats.pool_bases += (uint64_t)j.q_len;
        } else load[g].empty_rows++;
        L.pieces.push_back(d);
    }
    if (link_len + ins_cap >= (1ull << 27) || link_len >= (1ull << 20)) return;  // beyond the packed tag's column field / the record's row field
    P.link_len = (uint32_t)link_len;
    P.out_cap = (uint32_t)(2 * link_len + 64);
    P.cell_off = L.cell_rows * 6, P.out_off = L.out_bytes;
    L.out_bytes += P.out_cap;
    P.first_job = (uint32_t)L.jobs.size();
    std::vector<LqJobCut> cuts;
    cut_lq_jobs(load, hooks_of<LqHooks>().job_cols, kLqRoundRows, L.hdr_words, L.lnk_words, cuts);
    for (const LqJobCut &c : cuts) {
        LqJobDev jb;
        memset(&jb, 0, sizeof(jb));
        jb.pile = (uint32_t)r, jb.g_a = c.g_a, jb.g_b = c.g_b, jb.t0 = c.t0, jb.t1 = c.t1;
        jb.row_cap = c.row_cap, jb.lnk_cap = c.lnk_cap, jb.hdr_off = c.hdr_off, jb.lnk_off = c.lnk_off;
        P.row_cap += c.row_cap;
        L.jobs.push_back(jb);
    }
    P.n_jobs = (uint32_t)cuts.size();
    L.cell_rows += P.row_cap;
    L.usable[r] = 1;
}

// Every round of the call; the tasks are the context's own vector.
LqLayout DeviceAligner::State::layout_lq(LqRound **rounds, size_t n) {
    LqLayout L;
    L.piles.resize(n), L.usable.assign(n, 0);
    tasks.clear();
    size_t n_pieces = 0;
    for (size_t r = 0; r < n; r++) n_pieces += rounds[r]->pieces.size();
    L.pieces.reserve(n_pieces);
    for (size_t r = 0; r < n; r++) layout_lq_round(*rounds[r], r, L);
    return L;
}

// The sequence words (parallel): memcpy of what is packed already, packing of the rest.  false: a byte outside [ACGT].
bool DeviceAligner::State::pack_lq_pool(const LqLayout &L) {
    pool.assign(L.pool_words + kPoolPadWords, 0);  // (the kernels fetch up to five words from a sequence's last base on)
    std::atomic<int> bad_any{0};
    par_ranges(L.srcs.size(), host_threads, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            const LqSrc &x = L.srcs[i];
            if (x.words) memcpy(pool.data() + x.word_off, x.words, (((size_t)x.len + 15) / 16) * sizeof(uint32_t));
            else if (!pack_into(pool.data() + x.word_off, x.ascii, x.len)) bad_any = 1;
        }
    });
    return !bad_any.load();
}

// The buffers the layout sizes, then the forward / traceback chunks bounded by the trace budget (the column streams of every chunk
// stay resident; the traceback runs in segments where a launch holds long pairs -- regions of several kb).
std::vector<AlignChunk> DeviceAligner::State::reserve_lq(const LqLayout &L) {
    const size_t nt = tasks.size();
    d_pool.reserve(pool.size()), d_tasks.reserve(nt), d_outs.reserve(nt), d_ops.reserve(L.ops_words + 2);
    d_lq_piles.reserve(L.piles.size()), d_lq_pieces.reserve(L.pieces.size()), d_lq_rec.reserve(L.cell_rows * 6 + 6);
    d_lq_jobs.reserve(L.jobs.size() + 1), d_lq_hdr.reserve(L.hdr_words + 1);
    d_lq_lnk.reserve(L.lnk_words + 64);  // (K12b fetches a row's 64 link slots ahead)
    d_lq_out.reserve(L.out_bytes + 1), d_lq_tmp.reserve(L.cell_rows + 1), d_lq_bnd.reserve((L.jobs.size() + 1) * 4 * (size_t)kLqLinkCap);
    return plan_chunks(tasks.data(), nt);
}

// Five uploads, K7 / K8a chunk by chunk (an event bracket per kernel, read behind the one synchronisation), K12, the records, the
// piles as K12 left them (into L.piles) and their characters (returned) down.
std::vector<char> DeviceAligner::State::launch_lq(LqLayout &L, const std::vector<AlignChunk> &chunks) {
    hipStream_t st = stream;
    const size_t n = L.piles.size(), nt = tasks.size();
    h2d(d_pool.p, pool.data(), pool.size() * sizeof(uint32_t), st);
    h2d(d_tasks.p, tasks.data(), nt * sizeof(AlnTask), st);
    h2d(d_lq_piles.p, L.piles.data(), n * sizeof(LqPileDev), st);
    h2d(d_lq_pieces.p, L.pieces.data(), L.pieces.size() * sizeof(LqPieceDev), st);
    if (!L.jobs.empty()) h2d(d_lq_jobs.p, L.jobs.data(), L.jobs.size() * sizeof(LqJobDev), st);
    grow_lq_evs(2 * chunks.size() + 1);
    HIP_CHECK(hipEventRecord(lq_evs[0], st));
    for (size_t c = 0; c < chunks.size(); c++) {
        NDGPU_DBG(st, "lq: forward / traceback %zu..%zu of %zu tasks", chunks[c].begin, chunks[c].end, nt);
        launch_chunk(chunks[c], nullptr, nullptr, lq_evs[2 * c + 1], lq_evs[2 * c + 2], nullptr);
    }
    mark(kEvLqMsaBegin, st);
    NDGPU_DBG(st, "lq: msa of %zu piles", n);
    launch_lq_msa(d_lq_piles.p, d_lq_jobs.p, d_lq_pieces.p, d_tasks.p, d_outs.p, d_ops.p, d_pool.p, d_lq_hdr.p, d_lq_lnk.p, d_lq_rec.p,
                  d_lq_bnd.p, d_lq_tmp.p, d_lq_out.p, (int)n, (int)L.jobs.size(), hooks_of<LqHooks>().warm, hooks_of<LqHooks>().force_repair, st);
    mark(kEvLqMsaEnd, st);
    h_outs.reserve(nt + 1);
    HIP_CHECK(hipMemcpyAsync(h_outs.p, d_outs.p, nt * sizeof(AlnOut), hipMemcpyDeviceToHost, st));
    std::vector<char> out(L.out_bytes + 1);
    d2h(L.piles.data(), d_lq_piles.p, n * sizeof(LqPileDev), st);
    if (L.out_bytes) d2h(out.data(), d_lq_out.p, L.out_bytes, st);
    sync_drain(st);
    HIP_CHECK(hipGetLastError());
    return out;
}

// The kernels' times and counters, then round by round: taken (its walk string and its stats) or declined.
void DeviceAligner::State::tally_lq(LqRound **rounds, const LqLayout &L, size_t n_chunks, const std::vector<char> &out) {
    const size_t nt = tasks.size();
    for (size_t c = 0; c < n_chunks; c++) {
        stats.forward_ms += ms_between(lq_evs[2 * c], lq_evs[2 * c + 1]);
        stats.traceback_ms += ms_between(lq_evs[2 * c + 1], lq_evs[2 * c + 2]);
    }
    stats.forward_launches += n_chunks, stats.traceback_launches += n_chunks;
    stats.lq_ms += ms(kEvLqMsaBegin, kEvLqMsaEnd);
    stats.lq_launches++, stats.tasks += nt;
    tally_outs(nt, nullptr);  // (ST_NEED_WIDE is looked for piece by piece below)
    for (size_t r = 0; r < L.piles.size(); r++) {
        stats.lq_rounds++;
        const LqPileDev &P = L.piles[r];
        const LqPieceDev *pc = L.pieces.data() + P.first_piece;
        const uint32_t n_pc = L.usable[r] ? kLqRoundRows * P.n_regions : 0u;
        // (an alignment whose live band left the register path: K12 saw it as unaligned, so its pile goes the host way, where
        // run_chunk reruns it in the wide kernel)
        bool need_wide = false;
        for (uint32_t k = 0; k < n_pc && !need_wide; k++) need_wide = pc[k].task >= 0 && h_outs.p[pc[k].task].status == ST_NEED_WIDE;
        if (!L.usable[r] || need_wide || P.err != 0) {
            stats.lq_declined++;
            if (trace_on()) fprintf(stderr, "[ndgpu trace] K12 declined a pile (code %u): host path\n", L.usable[r] ? (need_wide ? 1u : P.err) : 9u);
            continue;
        }
        rounds[r]->lqc.assign(out.data() + P.out_off, P.out_len);
        rounds[r]->ok = true;
        stats.lq_repairs += P.n_repair, stats.lq_jobs += P.n_jobs, stats.lq_columns += P.link_len, stats.lq_out += P.out_len;
        for (uint32_t k = 0; k < n_pc; k++) {
            const int32_t t = pc[k].task;
            if (t < 0) continue;
            stats.lq_bases += (uint64_t)tasks[(size_t)t].q_len;
            if (h_outs.p[t].status == ST_ALIGNED) stats.lq_aln_columns += (uint64_t)h_outs.p[t].n_cols;
        }
    }
}

void DeviceAligner::run_lq(LqRound **rounds, size_t n) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    const uint64_t tc0 = wall_ns();
    LqLayout L = S.layout_lq(rounds, n);
    const size_t nt = S.tasks.size();
    if (nt == 0) {  // nothing K12 takes in this call: every pile goes the host way
        S.stats.lq_rounds += n, S.stats.lq_declined += n;
        return;
    }
    // bytes outside [ACGT]: the host path reports them.  (This exit counts neither lq_rounds nor lq_declined, unlike the one above
    // and unlike a round that is not usable: kept as it is, the counters do not move in a change of the code's shape.)
    if (!S.pack_lq_pool(L)) return;
    const std::vector<AlignChunk> chunks = S.reserve_lq(L);
    const uint64_t tc1 = wall_ns();
    const std::vector<char> out = S.launch_lq(L, chunks);
    const uint64_t tc2 = wall_ns();
    S.tally_lq(rounds, L, chunks.size(), out);
    g_prof.c_pack += tc1 - tc0, g_prof.c_dev += tc2 - tc1, g_prof.c_decode += wall_ns() - tc2, g_prof.c_jobs += nt;
}

void DeviceAligner::begin_batch(uint64_t order, bool reserved) { s_->batch_mu.lock(order, reserved); }
void DeviceAligner::reserve_batches(uint64_t order) { s_->batch_mu.reserve(order); }
void DeviceAligner::unreserve_batches(uint64_t order) { s_->batch_mu.unreserve(order); }
uint64_t DeviceAligner::next_order() {
    static std::atomic<uint64_t> n{1};
    return n.fetch_add(1);
}
void DeviceAligner::end_batch() { s_->batch_mu.unlock(); }

// ---- the main phase of a batch of piles, entirely on the device.  run_main (below) is the sequence of these steps:
//   layout (layout_piles) -> align: K7 forward, K8a traceback (align_main) -> tags: K8s shift scan, accept, K8b tags, column scan
//   (launch_tags) -> [one host sync: exact cell / link totals] -> plan (plan_msa) -> links + scoring: K9, K10 + walk
//   (count_and_score) -> stats (tally_main) -> unpack (unpack_paths).  Where every pile of the launch asks for it, K20 takes the
//   walks: plan_cns behind the plan, launch_cns inside count_and_score, fetch_cns instead of unpack (see the K20 section below).
// A step reads what it is given and returns one result; pool, tasks, reads and piles are the context's own vectors (reads and
// piles stay alive to end_batch: run_extract's kernels read their device copies).

// Fills the context's pool, tasks, reads and piles from the callers' piles; returns the rest of the layout.
MainLayout DeviceAligner::State::layout_piles(MainPile **mp, size_t np) {
    MainLayout L;
    pool.clear();
    tasks.clear();
    reads.clear();
    piles.assign(np, PileDev());
    L.bad_pile.assign(np, 0);
    for (size_t p = 0; p < np; p++) {
        MainPile &M = *mp[p];
        PileDev &P = piles[p];
        M.path.clear();
        M.slot = (int)p;
        memset(&P, 0, sizeof(P));
        P.seed_len = M.aln_end[0] + 1;
        P.n_reads = M.n;
        P.first_read = (uint32_t)reads.size();
        P.min_len_aln = M.min_len_aln;
        P.max_cov_aln = M.max_cov_aln;
        P.factor = M.factor;
        P.col_off = L.col_slots;
        L.col_slots += (uint64_t)P.seed_len + 1;
        P.acc_off = L.acc_slots;
        L.acc_slots += M.n;
        if (M.dev_off) P.seed_off = (uint64_t)M.dev_off[0] | kOffDb;
        else {
            P.seed_off = (uint64_t)pool.size() * 16;
            if (!pack_append(pool, M.seqs[0], M.seq_len[0])) L.bad_pile[p] = 1;
            stats.pool_bases += M.seq_len[0];
        }
        for (unsigned i = 0; i < M.n; i++) {
            ReadDev R;
            memset(&R, 0, sizeof(R));
            R.aln_start = M.aln_start[i];
            R.aln_end = M.aln_end[i];
            uint64_t tag_cap, ci_cap;
            if (i == 0) {
                R.task = -1;
                tag_cap = ci_cap = P.seed_len;
            } else {
                AlnTask t;
                memset(&t, 0, sizeof(t));
                t.q_len = (int32_t)M.seq_len[i];
                t.t_len = (int32_t)(M.aln_end[i] - M.aln_start[i] + 1);
                if (M.dev_off) t.q_off = (uint64_t)M.dev_off[i] | kOffDb;
                else {
                    t.q_off = (uint64_t)pool.size() * 16;
                    if (!pack_append(pool, M.seqs[i], M.seq_len[i])) L.bad_pile[p] = 1;
                    stats.pool_bases += M.seq_len[i];
                }
                t.t_off = P.seed_off + M.aln_start[i];
                task_limits(t, M.hq, L.ops_words, stats);
                R.task = (int32_t)tasks.size();
                tasks.push_back(t);
                tag_cap = t.ops_cap;
                ci_cap = (uint64_t)t.t_len;
            }
            R.tag_off = L.tag_slots;
            L.tag_slots += tag_cap;
            R.colidx_off = L.colidx_slots;
            L.colidx_slots += ci_cap + 1;
            reads.push_back(R);
            L.read_pile.push_back((uint32_t)p);
        }
        if (L.bad_pile[p]) {  // bytes outside [ACGT]: nothing of this pile is aligned
            fprintf(stderr, "[ndgpu] pile with bytes outside [ACGT]: reported as uncorrectable\n");
            for (uint32_t r = P.first_read + 1; r < reads.size(); r++) tasks[reads[r].task].max_d = 0;
            P.min_len_aln = 0xffffffffu;
        }
    }
    pool.insert(pool.end(), kPoolPadWords, 0u);
    if (L.tag_slots + 9 >= kTagSlotLimit) throw DeviceOom{(size_t)L.tag_slots * sizeof(uint32_t)};  // (halved like a sub-batch that does not fit)
    return L;
}

// The device (and pinned) buffers the layout sizes.
void DeviceAligner::State::reserve_layout(const MainLayout &L, size_t np) {
    const size_t nt = tasks.size(), nr = reads.size();
    d_pool.reserve(pool.size());
    d_tasks.reserve(nt + 1);
    d_outs.reserve(nt + 1);
    h_outs.reserve(nt + 1);
    d_ops.reserve(L.ops_words + 2);
    d_reads.reserve(nr);
    d_piles.reserve(np);
    d_read_pile.reserve(nr);
    d_acc.reserve(L.acc_slots + 1);
    d_tags.reserve(L.tag_slots + 9);  // (K9 reads 32-byte windows: up to 7 tags past a read's last one)
    d_colidx.reserve(L.colidx_slots + 1);
    d_cov.reserve(3 * (L.col_slots + 1));  // per column: coverage, insertion count, longest insertion -- three arrays in one block
    d_cellbase.reserve(L.col_slots + 1);
    d_entbase.reserve(L.col_slots + 1);
    d_err.reserve(kErrWords);
}

// Tasks [a, a + m) longest alignments first (their chains bound the launch), as a device list of ids relative to a -- or nullptr
// (table order) for a short chunk or under NDGPU_K7_NO_ORDER.  A counting sort over 64-base length classes: a sub-batch holds up
// to a million tasks and this runs on the context's critical path.
const int32_t *DeviceAligner::State::length_order(size_t a, size_t m) {
    if (!hooks_of<MainHooks>().k7_order || m <= 64) return nullptr;
    order.resize(m);
    order_cls.assign(kLenClasses + 1, 0);
    auto cls_of = [&](size_t i) {
        const uint32_t c = ((uint32_t)tasks[a + i].q_len + (uint32_t)tasks[a + i].t_len) >> 6;
        return (kLenClasses - 1) - std::min<uint32_t>(c, kLenClasses - 1);  // class 0 = the longest
    };
    for (size_t i = 0; i < m; i++) order_cls[cls_of(i) + 1]++;
    for (uint32_t c = 0; c < kLenClasses; c++) order_cls[c + 1] += order_cls[c];
    for (size_t i = 0; i < m; i++) order[order_cls[cls_of(i)]++] = (int32_t)i;
    d_ids.reserve(m);
    h2d(d_ids.p, order.data(), m * sizeof(int32_t), stream);
    return d_ids.p;
}

// K7 / K8a chunk by chunk, the AlnOut records to the host, the wide-band tasks run again.
void DeviceAligner::State::align_main(const std::vector<AlignChunk> &chunks, size_t np) {
    hipStream_t st = stream;
    const size_t nt = tasks.size();
    for (const AlignChunk &ch : chunks) {
        NDGPU_DBG(st, "main: forward %zu..%zu of %zu tasks, %zu piles", ch.begin, ch.end, nt, np);
        const int32_t *ids = length_order(ch.begin, ch.end - ch.begin);
        // (K8a stays in table order: measured in round 5, the 64 walks of a wavefront ordered longest first like K7's --
        // equal lengths, long walks first -- cost 605 ms of traceback per step against 496: the lanes of a wavefront in pile
        // order walk neighbouring windows of one seed and share its cache lines; NDGPU_K8_ORDER=1 switches the order on)
        mark(kEvMainK7, st);
        launch_chunk(ch, ids, hooks_of<MainHooks>().k8_order ? ids : nullptr, evs[kEvMainK8a], evs[kEvMainAligned], "main");
        NDGPU_DBG(st, "main: traceback done");
        HIP_CHECK(hipEventSynchronize(evs[kEvMainAligned]));  // (chunk by chunk: the next one records the same three events)
        stats.forward_ms += ms(kEvMainK7, kEvMainK8a);
        stats.forward_launches++;
        stats.traceback_ms += ms(kEvMainK8a, kEvMainAligned);
        stats.traceback_launches++;
    }
    if (!nt) return;
    HIP_CHECK(hipMemcpyAsync(h_outs.p, d_outs.p, nt * sizeof(AlnOut), hipMemcpyDeviceToHost, st));
    sync_drain(st);
    std::vector<int32_t> wide;
    tally_outs(nt, &wide);  // (before run_wide: a wide task counts with what the register path reported)
    if (!wide.empty()) run_wide(false, wide);
    stats.tasks += nt;
}

// The four launches between the events kEvTagsBegin and kEvTagsEnd: shift scan, accept, tags, column scan.
void DeviceAligner::State::launch_tags(const CovPlanes &cov, size_t np) {
    hipStream_t st = stream;
    const int nr = (int)reads.size();
    mark(kEvTagsBegin, st);
    NDGPU_DBG(st, "main: shift_scan");
    launch_shift_scan(d_tasks.p, d_outs.p, d_ops.p, d_reads.p, nr, st);
    NDGPU_DBG(st, "main: pile_accept");
    launch_pile_accept(d_piles.p, d_reads.p, d_acc.p, cov.cov, (int)np, st);
    NDGPU_DBG(st, "main: make_tags");
    launch_make_tags(d_piles.p, d_reads.p, d_tasks.p, d_ops.p, d_pool.p, db_pool, d_read_pile.p, d_tags.p, d_colidx.p, cov.inscnt,
                     cov.insmax, nr, st);
    NDGPU_DBG(st, "main: col_scan");
    launch_col_scan(d_piles.p, cov.cov, cov.inscnt, cov.insmax, d_cellbase.p, d_entbase.p, (int)np, st);
    NDGPU_DBG(st, "main: col_scan done");
    mark(kEvTagsEnd, st);
}

// From the piles as the column scan left them (n_cells, n_tags, err): every pile's K10 segments -- `seg_len` columns each, the
// last one takes the remainder -- on the work list of its tier, its offsets into the cell / link / path tables, K9's column
// blocks.  Pure host arithmetic; writes the piles' n_seg, seg_off, n_repair, tier and the three offsets.
static MsaPlan plan_msa(std::vector<PileDev> &piles) {
    const MainHooks &k = hooks_of<MainHooks>();
    MsaPlan M;
    for (size_t p = 0; p < piles.size(); p++) {
        PileDev &P = piles[p];
        if (k.k10_large) P.err = 3;
        if (k.k10_slow) P.err = 2;
        P.n_seg = std::max<uint32_t>(1u, (uint32_t)(((uint64_t)P.seed_len + k.k10_seg_len / 2) / k.k10_seg_len));
        P.seg_off = M.n_segs;
        M.n_segs += P.n_seg;
        P.n_repair = 0;
        P.tier = P.err == 3 ? 1u : 0u;
        std::vector<SegItem> &dst = P.err == 2 ? M.items_slow : P.err == 3 ? M.items_large : M.items_small;
        for (uint32_t g = 0; g < P.n_seg; g++) dst.push_back(SegItem{(uint32_t)p, g});
    }
    for (size_t p = 0; p < piles.size(); p++) {
        PileDev &P = piles[p];
        P.cell_off = M.cells;
        P.ent_off = M.ents;
        P.path_off = M.paths;
        M.cells += P.n_cells;
        M.ents += P.n_tags;
        M.paths += P.n_cells / 6 + 1;
        for (uint32_t c = 0; c < P.seed_len; c += kColBlock) M.blocks.push_back(ColBlock{(uint32_t)p, c});
    }
    return M;
}

// The tables K9 / K10 fill, sized by the plan; its column blocks and the three item lists (small | large | slow) go up.
void DeviceAligner::State::upload_plan(const MsaPlan &plan) {
    hipStream_t st = stream;
    d_cell_start.reserve(plan.cells + 1);
    d_cell_len.reserve(plan.cells + 1);
    d_cell_bpp.reserve(plan.cells + 1);
    d_cell_blink.reserve(plan.cells + 1);
    d_ent_pp.reserve(plan.ents + 1);
    d_ent_ppp.reserve(plan.ents + 1);
    d_ent_cnt.reserve(plan.ents + 1);
    // (d_ent_score, 8 bytes per link, belongs to the int64 kernel: allocated only when a pile needs it -- see the rescue pass)
    d_path.reserve(plan.paths + 1);
    d_blocks.reserve(plan.blocks.size() + 1);
    d_cell_best.reserve(plan.cells + 1);
    d_sums.reserve(plan.n_segs + 1);
    d_spec.reserve((size_t)plan.n_segs * kSegEnts + 1);
    d_fin.reserve((size_t)plan.n_segs * kSegEnts + 1);
    d_items.reserve(plan.n_items() + 1);
    d_bt_exit.reserve((size_t)plan.n_segs * kBtSlots + 1);
    d_bt_steps.reserve((size_t)plan.n_segs * kBtSlots + 1);
    d_bt_entry.reserve(plan.n_segs + 1);
    d_bt_off.reserve(plan.n_segs + 1);
    h2d(d_blocks.p, plan.blocks.data(), plan.blocks.size() * sizeof(ColBlock), st);
    h2d(d_items.p, plan.items_small.data(), plan.items_small.size() * sizeof(SegItem), st);
    h2d(d_items.p + plan.items_small.size(), plan.items_large.data(), plan.items_large.size() * sizeof(SegItem), st);
    h2d(d_items.p + plan.items_small.size() + plan.items_large.size(), plan.items_slow.data(), plan.items_slow.size() * sizeof(SegItem), st);
}

// K10 + the best_pp walk behind one attempt of K9 (events kEvScoreBegin .. kEvWalkBegin .. kEvWalkEnd).  A sub-batch small enough for the reserved compute units
// (4 two-wave blocks each) scores there: fork from the context's stream before, join behind.
void DeviceAligner::State::score_pass(const MsaPlan &plan, const K10Args &k10) {
    hipStream_t st = stream;
    const size_t np = piles.size();
    const bool on_reserved = lat_stream && np <= (size_t)reserved_cus * 2;
    hipStream_t sst = on_reserved ? lat_stream : st;
    if (on_reserved) {
        HIP_CHECK(hipEventRecord(ev_lat0, st));
        HIP_CHECK(hipStreamWaitEvent(sst, ev_lat0, 0));
        mark(kEvScoreBegin, sst);
    }
    launch_score_backtrack(k10, d_items.p, (int)plan.items_small.size(), d_items.p + plan.items_small.size(), (int)plan.items_large.size(),
                           d_items.p, (int)plan.n_items(), d_ent_score.cap >= plan.ents + 1 ? d_ent_score.p : nullptr, false, d_path.p,
                           d_bt_exit.p, d_bt_steps.p, d_bt_entry.p, d_bt_off.p, (int)np, sst, evs[kEvWalkBegin], on_reserved ? nullptr : stream2,
                           ev_fork, ev_join);
    mark(kEvWalkEnd, sst);
    NDGPU_DBG(st, "main: score + walk done");
    if (on_reserved) {
        HIP_CHECK(hipEventRecord(ev_lat1, sst));
        HIP_CHECK(hipStreamWaitEvent(st, ev_lat1, 0));
    }
}

// The piles the segment kernels handed to the int64 HBM-resident kernel (err == 2: a column wider than the LDS tables, raw scores
// out of the int32 working range) when its 8-byte-per-link score array was not there yet: that kernel and the walk, once more.
void DeviceAligner::State::rescue_pass(const MsaPlan &plan, const K10Args &k10) {
    d_ent_score.reserve(plan.ents + 1);
    launch_score_backtrack(k10, nullptr, 0, nullptr, 0, d_items.p, (int)plan.n_items(), d_ent_score.p, true, d_path.p, d_bt_exit.p,
                           d_bt_steps.p, d_bt_entry.p, d_bt_off.p, (int)piles.size(), stream, nullptr, nullptr, nullptr, nullptr);
}

// NDGPU_K9_DIGEST: a digest of the tables an attempt of K9 left, for comparing two builds or two paths of K9.  The stream is idle
// here; the kernel, its four words and their copy exist only under the switch.
void DeviceAligner::State::k9_digest_trace(const K9Args &k9, size_t np) {
    hipStream_t st = stream;
    unsigned long long *d_dig = nullptr, dig[4] = {};
    HIP_CHECK(hipMalloc((void **)&d_dig, sizeof(dig)));
    HIP_CHECK(hipMemsetAsync(d_dig, 0, sizeof(dig), st));
    launch_k9_digest(k9, d_dig, (int)np, st);
    HIP_CHECK(hipMemcpyAsync(dig, d_dig, sizeof(dig), hipMemcpyDeviceToHost, st));
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipFree(d_dig));
    fprintf(stderr, "[ndgpu trace] K9 tables: digest=%016llx cells=%llu links=%llu max_cell_len=%llu\n", dig[0], dig[1], dig[2], dig[3]);
}

// Links and scores, up to three times: attempt 0 counts links with the small LDS lists; a cell with more distinct links than they
// hold raises err[0] and the sub-batch is counted and scored again with the full capacity (everything the kernels write is
// rewritten), and if that overflows too, a third time with the lists in device memory, which cannot (nd_device.h: kLinkCap).
// Returns the last attempt's error words, its piles and a view of its paths in the download arena.
MsaResult DeviceAligner::State::count_and_score(const MsaPlan &plan, const CovPlanes &cov, const CnsPlan *cns) {
    const MainHooks &hooks = hooks_of<MainHooks>();
    hipStream_t st = stream;
    const K9Args k9{d_piles.p,   d_reads.p,      d_acc.p,      d_blocks.p, d_tags.p,    d_colidx.p,  cov.insmax, d_cellbase.p,
                    d_entbase.p, d_cell_start.p, d_cell_len.p, d_ent_pp.p, d_ent_ppp.p, d_ent_cnt.p, d_err.p};
    K10Args k10 = k10_args_from(k9);
    k10.coverage = cov.cov;
    k10.cell_best_pp = d_cell_bpp.p, k10.cell_best_link = d_cell_blink.p, k10.cell_best = d_cell_best.p;
    k10.sums = d_sums.p, k10.spec = d_spec.p, k10.fin = d_fin.p;
    k10.seg_len = hooks.k10_seg_len, k10.warm = hooks.k10_warm, k10.guard = hooks.k10_guard, k10.force_repair = hooks.k10_force_repair;
    const size_t np = piles.size();
    // what an attempt brings down: the piles, and either their walks or -- cns: K20 runs on the walks where bt_emit left them, in
    // front of the synchronisation (the retry / rescue decision needs it anyway), so that its records ride down with the piles
    static_assert(sizeof(CnsWalkOutDev) == sizeof(CnsOutDev), "K20's and K21's records ride down in the same room");
    const size_t down_bytes = np * sizeof(PileDev) + (cns ? np * sizeof(CnsOutDev) + 256 : plan.paths * sizeof(PathItem)) + 1024;
    MsaResult R;
    R.piles.resize(np);
    if (cns && cns->walk) R.cnsw.resize(np);
    else if (cns) R.cns.resize(np);
    const void *v_cns = nullptr;
    auto walks_down = [&] {  // behind the walk: K20's records, or the walks themselves
        if (cns && cns->walk) {
            launch_cns_walk_jobs(*cns, d_piles.p, d_path.p);
            v_cns = d2h(nullptr, d_cnsw_out.p, np * sizeof(CnsWalkOutDev), st);
            stats.cnsw_d2h_bytes += np * sizeof(CnsWalkOutDev);
        } else if (cns) {
            launch_cns(*cns, d_piles.p, d_path.p);
            v_cns = d2h(nullptr, d_cns_out.p, np * sizeof(CnsOutDev), st);
            stats.cns_d2h_bytes += np * sizeof(CnsOutDev);
        } else {
            R.hpath = (const PathItem *)d2h(nullptr, d_path.p, plan.paths * sizeof(PathItem), st);
            stats.walk_d2h_bytes += plan.paths * sizeof(PathItem);
        }
    };
    auto walks_landed = [&] {
        if (!cns) return;
        if (cns->walk) {
            memcpy(R.cnsw.data(), v_cns, np * sizeof(CnsWalkOutDev));
            stats.cnsw_ms += ms(kEvCnswBegin, kEvCnswEnd);
            return;
        }
        memcpy(R.cns.data(), v_cns, np * sizeof(CnsOutDev));
        stats.cns_ms += ms(kEvCnsBegin, kEvCnsEnd);
    };
    for (int attempt = hooks.k9_full ? 1 : 0, first = 1; attempt < 3; attempt++, first = 0) {
        reserve_down(down_bytes, st);
        h2d(d_piles.p, piles.data(), np * sizeof(PileDev), st);
        if (!first) HIP_CHECK(hipMemsetAsync(d_err.p, 0, kErrWords * sizeof(uint32_t), st));
        mark(kEvLinksBegin, st);
        NDGPU_DBG(st, "main: count_links %zu blocks, cells %llu ents %llu segs %u", plan.blocks.size(), (unsigned long long)plan.cells,
                  (unsigned long long)plan.ents, plan.n_segs);
        if (attempt < 2) {
            launch_count_links(k9, (int)plan.blocks.size(), attempt != 0, st);
        } else {  // (the stream is idle here: the attempt before was waited for)
            uint32_t cap = 1;
            for (size_t p = 0; p < np; p++) cap = std::max(cap, piles[p].n_acc);
            const int grid = (int)std::min<size_t>(plan.blocks.size(), (size_t)kLinkGlobalGrid);
            d_link_lists.reserve((size_t)grid * 18u * cap + 1);
            launch_count_links_global(k9, d_link_lists.p, cap, (int)plan.blocks.size(), grid, st);
        }
        mark(kEvScoreBegin, st);
        NDGPU_DBG(st, "main: score + walk");
        score_pass(plan, k10);
        const void *v_piles = d2h(nullptr, d_piles.p, np * sizeof(PileDev), st);  // (re-taken by the rescue pass)
        walks_down();
        const void *v_err = d2h(nullptr, d_err.p, sizeof(R.herr), st);
        HIP_CHECK(hipStreamSynchronize(st));
        HIP_CHECK(hipGetLastError());
        memcpy(R.piles.data(), v_piles, np * sizeof(PileDev));
        memcpy(R.herr, v_err, sizeof(R.herr));
        walks_landed();
        bool rescue = false;
        for (size_t p = 0; p < np; p++) rescue = rescue || R.piles[p].err == 2;
        if (rescue) {
            rescue_pass(plan, k10);
            reserve_down(down_bytes, st);
            v_piles = d2h(nullptr, d_piles.p, np * sizeof(PileDev), st);
            walks_down();
            HIP_CHECK(hipStreamSynchronize(st));
            HIP_CHECK(hipGetLastError());
            memcpy(R.piles.data(), v_piles, np * sizeof(PileDev));
            walks_landed();
        }
        if (attempt < 2 && trace_on())
            fprintf(stderr, "[ndgpu trace] K9 blocks: compact %u (max cover %u), fallback %u (min cover %u)\n", R.herr[1], R.herr[3], R.herr[2],
                    R.herr[4] ? ~R.herr[4] : 0u);
        if (hooks.k9_digest) k9_digest_trace(k9, np);
        if (attempt == 0 ? !R.herr[0] && !hooks.k9_force_retry : !R.herr[0]) break;
        if (attempt == 2) break;  // (cannot happen: the lists hold one entry per accepted read)
        k9_retries++;
        if (trace_on()) {
            if (attempt == 0) fprintf(stderr, "[ndgpu trace] K9: a cell holds more than %d distinct links, sub-batch repeated with %d\n", kLinkCapSmall, kLinkCap);
            else fprintf(stderr, "[ndgpu trace] K9: a cell holds more than %d distinct links, sub-batch repeated with the lists in device memory\n", kLinkCap);
        }
    }
    return R;
}

// The main phase's counters and the NDGPU_TRACE line, both from one reading of each event pair.  piles: as the last attempt left
// them; tp: wall clock at the start of run_main and behind its prep, align, tags and msa parts.
void DeviceAligner::State::tally_main(const MsaPlan &plan, const std::vector<uint8_t> &bad_pile, MainPile **mp, const uint64_t tp[5]) {
    const size_t np = piles.size();
    const double t_tags = ms(kEvTagsBegin, kEvTagsEnd), t_links = ms(kEvLinksBegin, kEvScoreBegin), t_score = ms(kEvScoreBegin, kEvWalkBegin),
                 t_back = ms(kEvWalkBegin, kEvWalkEnd);
    stats.tags_ms += t_tags;
    stats.links_ms += t_links;
    stats.score_ms += t_score;
    stats.score_launches++;
    stats.backtrack_ms += t_back;
    if (trace_on()) {
        uint32_t longest = 0, rep = 0, slow = 0;
        for (size_t p = 0; p < np; p++) {
            longest = std::max(longest, piles[p].seed_len);
            if (piles[p].n_repair == 0xffffffffu) slow++;
            else rep += piles[p].n_repair;
        }
        fprintf(stderr, "[ndgpu trace] run_main %zu piles longest %u | host prep %.1f align %.1f tags %.1f msa %.1f ms | K9 %.1f K10 %.1f backtrack %.1f ms | %u segments, %u repaired, %u piles through the int64 kernel\n",
                np, longest, (tp[1] - tp[0]) * 1e-6, (tp[2] - tp[1]) * 1e-6, (tp[3] - tp[2]) * 1e-6, (tp[4] - tp[3]) * 1e-6, t_links, t_score, t_back,
                plan.n_segs, rep, slow);
    }
    for (size_t p = 0; p < np; p++) {
        const PileDev &P = piles[p];
        mp[p]->n_aligned = P.n_acc;
        if (bad_pile[p]) continue;
        stats.path_items += P.path_len;
        stats.links += P.n_links;
        stats.score_segments += P.n_seg;
        if (P.n_repair == 0xffffffffu) stats.score_slow_piles++;  // marker left by the int64 kernel
        else stats.score_repairs += P.n_repair;
    }
}

static void unpack_walk(const PathItem *src, uint32_t len, MainPile &M) {
    M.path.resize(len);
    for (uint32_t k = 0; k < len; k++) {
        PathStep &d = M.path[k];
        d.t_pos = tag_tpos(src[k].tag);
        d.delta = (uint16_t)tag_delta(src[k].tag);
        d.base = (uint8_t)tag_base(src[k].tag);
        d.link = src[k].link;
        d.cov = src[k].cov;
    }
}

// The walk of every pile (one step per consensus position) into its MainPile: piles dealt to the context's host threads.
static void unpack_paths(const std::vector<PileDev> &piles, const PathItem *hpath, const std::vector<uint8_t> &bad_pile, MainPile **mp,
                         int host_threads) {
    const size_t np = piles.size();
    host_each(np, host_threads <= 1 || np < 4, host_threads, np, true, [&](size_t p) {
        if (bad_pile[p]) return;
        const PileDev &P = piles[p];
        MainPile &M = *mp[p];
        unpack_walk(hpath + P.path_off, P.path_len, M);
    });
}

// ---- K20: the walk's consensus words and low-quality windows on the device (nd_cns.h states the rule; DESIGN.md section 0a''''''''').
// In run_main: plan_cns (jobs and buffers, behind upload_plan) -> launch_cns inside count_and_score, behind every walk -> fetch_cns
// (exact-size copies of the dense words and windows; a declined pile's walk on its own, unpacked for the host routine).

// Test hook NDGPU_CNS_DECLINE=<k>: every k-th walk offered to K20 is left to the host routine (counted over the process).
static bool cns_decline_hook() {
    static const uint64_t k = env_u64("NDGPU_CNS_DECLINE", 0);
    static std::atomic<uint64_t> seen{0};
    return k && seen.fetch_add(1) % k == k - 1;
}
// Window slots of a walk of at most `items` items: recorded emissions lie at least 25 indices apart (msa_kernels.hip, K20).
static uint32_t cns_win_cap(uint64_t items) { return (uint32_t)(items / 24u + 1u); }

CnsPlan DeviceAligner::State::plan_cns(const MsaPlan &plan, MainPile **mp) {
    CnsPlan C;
    const size_t np = piles.size();
    C.jobs.resize(np);
    for (size_t p = 0; p < np; p++) {
        CnsJobDev &J = C.jobs[p];
        memset(&J, 0, sizeof(J));
        J.pile = (uint32_t)p;
        J.win_off = C.win_slots;
        J.n = piles[p].n_cells / 6 + 1;   // the capacity of the walk's slice (plan_msa): its length is not known yet
        J.win_cap = cns_win_cap(J.n);
        J.min_cov = mp[p]->min_cov;
        J.lq_max_len = mp[p]->lq_max_len;
        J.decline = cns_decline_hook() ? 1u : 0u;
        C.win_slots += J.win_cap;
    }
    d_cns_jobs.reserve(np);
    d_cns_out.reserve(np);
    d_cns_words.reserve(plan.paths + 1);
    d_cns_dense.reserve(plan.paths + 1);
    d_cns_wins.reserve(2 * C.win_slots + 2);
    d_cns_wdense.reserve(2 * C.win_slots + 2);
    h2d(d_cns_jobs.p, C.jobs.data(), np * sizeof(CnsJobDev), stream);
    return C;
}

void DeviceAligner::State::launch_cns(const CnsPlan &cns, const PileDev *dev_piles, const PathItem *dev_path) {
    hipStream_t st = stream;
    mark(kEvCnsBegin, st);
    NDGPU_DBG(st, "cns_windows: %zu walks", cns.jobs.size());
    launch_cns_windows(d_cns_jobs.p, dev_piles, dev_path, d_cns_words.p, d_cns_wins.p, d_cns_out.p, d_cns_dense.p, d_cns_wdense.p,
                       (int)cns.jobs.size(), st);
    mark(kEvCnsEnd, st);
    stats.cns_launches++;
}

void DeviceAligner::State::fetch_cns(const CnsPlan &cns, const MsaResult &res, const std::vector<uint8_t> &bad_pile, MainPile **mp) {
    hipStream_t st = stream;
    const size_t np = piles.size();
    uint64_t n_words = 0, n_wins = 0, walk_bytes = 0, visited = 0;
    size_t n_declined = 0;
    for (size_t p = 0; p < np; p++) {
        const CnsOutDev &O = res.cns[p];
        if (O.err) n_declined++, walk_bytes += ((size_t)piles[p].path_len * sizeof(PathItem) + 255) & ~(size_t)255;
        else n_words += O.len, n_wins += O.n_win, visited += O.visited;
    }
    reserve_down(n_words * 4 + n_wins * 8 + walk_bytes + 1024, st);
    const uint32_t *w = (const uint32_t *)d2h(nullptr, d_cns_dense.p, n_words * 4, st);
    const uint32_t *wn = (const uint32_t *)d2h(nullptr, d_cns_wdense.p, n_wins * 8, st);
    std::vector<const PathItem *> walks(np, nullptr);
    for (size_t p = 0; p < np; p++)
        if (res.cns[p].err && !bad_pile[p]) {   // declined: this pile's walk alone, for the host routine
            walks[p] = (const PathItem *)d2h(nullptr, d_path.p + piles[p].path_off, (size_t)piles[p].path_len * sizeof(PathItem), st);
            stats.walk_d2h_bytes += (size_t)piles[p].path_len * sizeof(PathItem);
        }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    stats.cns_d2h_bytes += n_words * 4 + n_wins * 8;
    for (size_t p = 0; p < np; p++) {
        MainPile &M = *mp[p];
        const CnsOutDev &O = res.cns[p];
        if (O.err) {
            if (bad_pile[p]) continue;
            if (O.err != kCnsErrHook) fprintf(stderr, "[ndgpu] cns_windows: a walk of %u items left to the host routine (error word %u)\n", piles[p].path_len, O.err);
            unpack_walk(walks[p], piles[p].path_len, M);
            stats.cns_declined++;
            continue;
        }
        if (!bad_pile[p]) {
            M.cns_words.assign(w, w + O.len);
            M.cns_windows.assign(wn, wn + 2 * (size_t)O.n_win);
            const uint32_t counts[5] = {O.len, O.uncorrected_len, O.lstrip, O.rstrip, O.lqseq_total_length};
            memcpy(M.cns_counts, counts, sizeof(counts));
            M.cns_ready = true;
            stats.cns_jobs++;
            stats.cns_regions += O.n_win;
        }
        w += O.len, wn += 2 * (size_t)O.n_win;
    }
    if (trace_on())
        fprintf(stderr, "[ndgpu trace] cns_windows %zu walks | K20 %.3f ms | %llu words, %llu windows, %zu declined | automaton stepped through %llu items (%.1f %% skipped idle)\n",
                np, ms(kEvCnsBegin, kEvCnsEnd), (unsigned long long)n_words, (unsigned long long)n_wins, n_declined, (unsigned long long)visited,
                n_words ? 100.0 * (double)(n_words - visited) / (double)n_words : 0.0);
}

// The batched entry's walks: the callers' steps go up as PathItems, K20 and its gather run as in run_main, the records come down,
// then the dense words and windows at exact size.  A declined walk keeps done == false.
void DeviceAligner::run_cns(CnsReq *reqs, size_t n) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    hipStream_t st = S.stream;
    constexpr size_t kCnsSliceJobs = 4096, kCnsSliceItems = (size_t)32 << 20;
    std::vector<PathItem> items;
    CnsPlan C;
    std::vector<CnsOutDev> outs;
    for (size_t a = 0; a < n;) {
        items.clear(), C.jobs.clear();
        C.win_slots = 0;
        size_t b = a;
        for (; b < n && b - a < kCnsSliceJobs; b++) {
            const CnsReq &rq = reqs[b];
            if (b > a && items.size() + rq.n > kCnsSliceItems) break;
            CnsJobDev J;
            memset(&J, 0, sizeof(J));
            J.path_off = items.size();
            J.n = (uint32_t)rq.n;
            J.win_off = C.win_slots;
            J.win_cap = cns_win_cap(rq.n);
            J.min_cov = rq.min_cov;
            J.lq_max_len = rq.lq_max_len;
            J.decline = cns_decline_hook() ? 1u : 0u;
            C.win_slots += J.win_cap;
            C.jobs.push_back(J);
            for (size_t k = 0; k < rq.n; k++) {
                const PathStep &s = rq.steps[k];
                PathItem it;
                it.tag = s.base == 4 ? 4u : tag_pack(s.t_pos, 0u, s.base);
                it.link = s.link, it.cov = s.cov;
                items.push_back(it);
            }
        }
        const size_t m = b - a;
        S.d_cns_jobs.reserve(m);
        S.d_cns_out.reserve(m);
        S.d_path.reserve(items.size() + 1);
        S.d_cns_words.reserve(items.size() + 1);
        S.d_cns_dense.reserve(items.size() + 1);
        S.d_cns_wins.reserve(2 * C.win_slots + 2);
        S.d_cns_wdense.reserve(2 * C.win_slots + 2);
        S.h2d(S.d_cns_jobs.p, C.jobs.data(), m * sizeof(CnsJobDev), st);
        S.h2d(S.d_path.p, items.data(), items.size() * sizeof(PathItem), st);
        S.launch_cns(C, nullptr, S.d_path.p);
        HIP_CHECK(hipGetLastError());
        outs.resize(m);
        S.d2h(outs.data(), S.d_cns_out.p, m * sizeof(CnsOutDev), st);
        S.sync_drain(st);
        S.stats.cns_ms += S.ms(State::kEvCnsBegin, State::kEvCnsEnd);
        uint64_t n_words = 0, n_wins = 0;
        for (const CnsOutDev &O : outs)
            if (!O.err) n_words += O.len, n_wins += O.n_win;
        S.reserve_down(n_words * 4 + n_wins * 8 + 1024, st);
        const uint32_t *w = (const uint32_t *)S.d2h(nullptr, S.d_cns_dense.p, n_words * 4, st);
        const uint32_t *wn = (const uint32_t *)S.d2h(nullptr, S.d_cns_wdense.p, n_wins * 8, st);
        HIP_CHECK(hipStreamSynchronize(st));
        S.stats.cns_d2h_bytes += m * sizeof(CnsOutDev) + n_words * 4 + n_wins * 8;
        for (size_t i = 0; i < m; i++) {
            CnsReq &rq = reqs[a + i];
            const CnsOutDev &O = outs[i];
            rq.done = !O.err;
            if (O.err) {
                S.stats.cns_declined++;
                continue;
            }
            rq.words.assign(w, w + O.len);
            rq.wins.assign(wn, wn + 2 * (size_t)O.n_win);
            const uint32_t counts[5] = {O.len, O.uncorrected_len, O.lstrip, O.rstrip, O.lqseq_total_length};
            memcpy(rq.counts, counts, sizeof(counts));
            w += O.len, wn += 2 * (size_t)O.n_win;
            S.stats.cns_jobs++;
            S.stats.cns_regions += O.n_win;
        }
        S.drain();
        if (trace_on())
            fprintf(stderr, "[ndgpu trace] cns_windows %zu walks (batched entry) | K20 %.3f ms | %llu words, %llu windows\n", m,
                    S.ms(State::kEvCnsBegin, State::kEvCnsEnd), (unsigned long long)n_words, (unsigned long long)n_wins);
        a = b;
    }
}

// ---- K21: the HiFi and -fast forms on the device (nd_cns.h states the rules; DESIGN.md section 0a'''''''''').  In run_main the
// steps are K20's: plan_cns_walk -> launch_cns_walk_jobs inside count_and_score -> fetch_cns_walk.  A launch goes to K21 when every
// pile asks and one of them is HiFi or -fast; a raw pile of such a launch is declined by the kernel (kCnsErrMode) and takes the host
// routine -- the engine's calls carry one set of arguments, so its launches do not mix raw piles with the others.

// Window slots of a HiFi walk of at most `items` items: emissions lie at least 6 indices apart (msa_kernels.hip, K21).
static uint32_t cns_walk_win_cap(uint64_t items) { return (uint32_t)(items / 6u + 1u); }

void DeviceAligner::State::reserve_cns_walk(const CnsPlan &C, size_t slots) {
    const size_t m = C.wjobs.size();
    d_cnsw_jobs.reserve(m);
    d_cnsw_out.reserve(m);
    d_cns_words.reserve(C.any_hifi ? slots + 1 : 1);
    d_cns_dense.reserve(C.any_hifi ? slots + 1 : 1);
    d_cns_wins.reserve(2 * C.win_slots + 2);
    d_cns_wdense.reserve(2 * C.win_slots + 2);
    d_cnsw_chars.reserve(C.any_fast ? slots + 1 : 1);
    d_cnsw_seq.reserve(C.any_fast ? slots + 1 : 1);
}

CnsPlan DeviceAligner::State::plan_cns_walk(const MsaPlan &plan, MainPile **mp) {
    CnsPlan C;
    C.walk = true;
    const size_t np = piles.size();
    C.wjobs.resize(np);
    for (size_t p = 0; p < np; p++) {
        CnsWalkJobDev &J = C.wjobs[p];
        memset(&J, 0, sizeof(J));
        J.pile = (uint32_t)p;
        J.mode = (uint32_t)mp[p]->cns_mode;
        J.n = piles[p].n_cells / 6 + 1;   // the capacity of the walk's slice (plan_msa)
        J.min_cov = mp[p]->min_cov;
        J.decline = cns_decline_hook() ? 1u : 0u;
        if (J.mode == kCnsModeHifi) {
            J.win_off = C.win_slots;
            J.win_cap = cns_walk_win_cap(J.n);
            C.win_slots += J.win_cap;
            C.any_hifi = true;
        } else if (J.mode == kCnsModeFast) C.any_fast = true;
    }
    reserve_cns_walk(C, plan.paths);
    d_cnsw_seed.reserve(1);
    h2d(d_cnsw_jobs.p, C.wjobs.data(), np * sizeof(CnsWalkJobDev), stream);
    return C;
}

void DeviceAligner::State::launch_cns_walk_jobs(const CnsPlan &cns, const PileDev *dev_piles, const PathItem *dev_path) {
    hipStream_t st = stream;
    mark(kEvCnswBegin, st);
    NDGPU_DBG(st, "cns_walk: %zu walks", cns.wjobs.size());
    launch_cns_walk(d_cnsw_jobs.p, dev_piles, dev_path, d_pool.p, db_pool, d_cnsw_seed.p, d_cns_words.p, d_cns_wins.p, d_cnsw_chars.p,
                    d_cnsw_out.p, d_cns_dense.p, d_cns_wdense.p, d_cnsw_seq.p, (int)cns.wjobs.size(), st);
    mark(kEvCnswEnd, st);
    stats.cnsw_launches++;
}

void DeviceAligner::State::fetch_cns_walk(const CnsPlan &cns, const MsaResult &res, const std::vector<uint8_t> &bad_pile, MainPile **mp) {
    hipStream_t st = stream;
    const size_t np = piles.size();
    uint64_t n_words = 0, n_wins = 0, n_bytes = 0, walk_bytes = 0;
    size_t n_mode[3] = {0, 0, 0}, n_declined = 0;
    for (size_t p = 0; p < np; p++) {
        const CnsWalkOutDev &O = res.cnsw[p];
        n_mode[cns.wjobs[p].mode < 3u ? cns.wjobs[p].mode : 0u]++;
        if (O.err) n_declined++, walk_bytes += ((size_t)piles[p].path_len * sizeof(PathItem) + 255) & ~(size_t)255;
        else n_words += O.n_words, n_wins += O.n_win, n_bytes += O.n_bytes;
    }
    reserve_down(n_words * 4 + n_wins * 8 + n_bytes + walk_bytes + 2048, st);
    const uint32_t *w = (const uint32_t *)d2h(nullptr, d_cns_dense.p, n_words * 4, st);
    const uint32_t *wn = (const uint32_t *)d2h(nullptr, d_cns_wdense.p, n_wins * 8, st);
    const char *sq = (const char *)d2h(nullptr, d_cnsw_seq.p, n_bytes, st);
    std::vector<const PathItem *> walks(np, nullptr);
    for (size_t p = 0; p < np; p++)
        if (res.cnsw[p].err && !bad_pile[p]) {   // declined: this pile's walk alone, for the host routine
            walks[p] = (const PathItem *)d2h(nullptr, d_path.p + piles[p].path_off, (size_t)piles[p].path_len * sizeof(PathItem), st);
            stats.walk_d2h_bytes += (size_t)piles[p].path_len * sizeof(PathItem);
        }
    HIP_CHECK(hipStreamSynchronize(st));
    HIP_CHECK(hipGetLastError());
    stats.cnsw_d2h_bytes += n_words * 4 + n_wins * 8 + n_bytes;
    for (size_t p = 0; p < np; p++) {
        MainPile &M = *mp[p];
        const CnsWalkOutDev &O = res.cnsw[p];
        const uint32_t mode = cns.wjobs[p].mode;
        if (O.err) {
            if (bad_pile[p]) continue;
            if (O.err != kCnsErrHook && O.err != kCnsErrMode)
                fprintf(stderr, "[ndgpu] cns_walk: a walk of %u items left to the host routine (error word %u)\n", piles[p].path_len, O.err);
            unpack_walk(walks[p], piles[p].path_len, M);
            if (mode == kCnsModeHifi) stats.cnsw_hifi_declined++;
            else if (mode == kCnsModeFast) stats.cnsw_fast_declined++;
            continue;
        }
        if (!bad_pile[p] && piles[p].path_len) {   // (a walk of no items: `path` stays empty and the engine ends the pile as ever)
            if (mode == kCnsModeHifi) {
                M.cns_words.assign(w, w + O.n_words);
                M.cns_windows.assign(wn, wn + 2 * (size_t)O.n_win);
                const uint32_t counts[5] = {O.len, 0, 0, 0, O.lqseq_total_length};
                memcpy(M.cns_counts, counts, sizeof(counts));
                stats.cnsw_hifi_jobs++;
                stats.cnsw_hifi_regions += O.n_win;
            } else {
                const uint32_t fast[4] = {O.lq_m, O.hq_m, O.lqseq_total_length, O.len};
                memcpy(M.cns_fast, fast, sizeof(fast));
                M.cns_seq.assign(sq, sq + O.n_bytes);
                stats.cnsw_fast_jobs++;
            }
            M.cns_ready = true;
        }
        w += O.n_words, wn += 2 * (size_t)O.n_win, sq += O.n_bytes;
    }
    if (trace_on())
        fprintf(stderr, "[ndgpu trace] cns_walk %zu walks: %zu HiFi, %zu -fast, %zu raw (left to the host) | K21 %.3f ms | %llu words, %llu windows, %llu bytes, %zu declined\n",
                np, n_mode[1], n_mode[2], n_mode[0], ms(kEvCnswBegin, kEvCnswEnd), (unsigned long long)n_words, (unsigned long long)n_wins,
                (unsigned long long)n_bytes, n_declined);
}

// The batched entry's walks of modes 1 and 2: steps up as PathItems, the HiFi seeds as byte codes, K21 and its gather, the records
// down, then words, windows and strings at exact size (the strings unpadded, one behind the other).  A declined walk keeps done == false.
void DeviceAligner::run_cns_walk(CnsWalkReq *reqs, size_t n) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    hipStream_t st = S.stream;
    constexpr size_t kSliceJobs = 4096, kSliceItems = (size_t)32 << 20;
    std::vector<PathItem> items;
    std::vector<uint8_t> seeds;
    CnsPlan C;
    C.walk = true;
    std::vector<CnsWalkOutDev> outs;
    for (size_t a = 0; a < n;) {
        items.clear(), seeds.clear(), C.wjobs.clear();
        C.win_slots = 0;
        C.any_hifi = C.any_fast = false;
        size_t b = a;
        for (; b < n && b - a < kSliceJobs; b++) {
            const CnsWalkReq &rq = reqs[b];
            if (b > a && (items.size() + rq.n > kSliceItems || seeds.size() + rq.seed_len > kSliceItems)) break;
            CnsWalkJobDev J;
            memset(&J, 0, sizeof(J));
            J.path_off = items.size();
            J.n = (uint32_t)rq.n;
            J.mode = (uint32_t)rq.mode;
            J.min_cov = rq.min_cov;
            J.decline = cns_decline_hook() ? 1u : 0u;
            if (J.mode == kCnsModeHifi) {
                J.win_off = C.win_slots;
                J.win_cap = cns_walk_win_cap(rq.n);
                C.win_slots += J.win_cap;
                J.seed_off = seeds.size();
                J.seed_len = (uint32_t)rq.seed_len;
                seeds.insert(seeds.end(), rq.seed_codes, rq.seed_codes + rq.seed_len);
                C.any_hifi = true;
            } else C.any_fast = true;
            C.wjobs.push_back(J);
            for (size_t k = 0; k < rq.n; k++) {
                const PathStep &s = rq.steps[k];
                PathItem it;
                it.tag = s.base == 4 ? 4u : tag_pack(s.t_pos, 0u, s.base);
                it.link = s.link, it.cov = s.cov;
                items.push_back(it);
            }
        }
        const size_t m = b - a;
        S.d_path.reserve(items.size() + 1);
        S.reserve_cns_walk(C, items.size());
        S.d_cnsw_seed.reserve(seeds.size() + 1);
        S.h2d(S.d_cnsw_jobs.p, C.wjobs.data(), m * sizeof(CnsWalkJobDev), st);
        S.h2d(S.d_path.p, items.data(), items.size() * sizeof(PathItem), st);
        S.h2d(S.d_cnsw_seed.p, seeds.data(), seeds.size(), st);
        S.launch_cns_walk_jobs(C, nullptr, S.d_path.p);
        HIP_CHECK(hipGetLastError());
        outs.resize(m);
        S.d2h(outs.data(), S.d_cnsw_out.p, m * sizeof(CnsWalkOutDev), st);
        S.sync_drain(st);
        S.stats.cnsw_ms += S.ms(State::kEvCnswBegin, State::kEvCnswEnd);
        uint64_t n_words = 0, n_wins = 0, n_bytes = 0;
        for (const CnsWalkOutDev &O : outs)
            if (!O.err) n_words += O.n_words, n_wins += O.n_win, n_bytes += O.n_bytes;
        S.reserve_down(n_words * 4 + n_wins * 8 + n_bytes + 2048, st);
        const uint32_t *w = (const uint32_t *)S.d2h(nullptr, S.d_cns_dense.p, n_words * 4, st);
        const uint32_t *wn = (const uint32_t *)S.d2h(nullptr, S.d_cns_wdense.p, n_wins * 8, st);
        const char *sq = (const char *)S.d2h(nullptr, S.d_cnsw_seq.p, n_bytes, st);
        HIP_CHECK(hipStreamSynchronize(st));
        S.stats.cnsw_d2h_bytes += m * sizeof(CnsWalkOutDev) + n_words * 4 + n_wins * 8 + n_bytes;
        size_t n_mode[3] = {0, 0, 0};
        for (size_t i = 0; i < m; i++) {
            CnsWalkReq &rq = reqs[a + i];
            const CnsWalkOutDev &O = outs[i];
            const bool hifi = rq.mode == (int)kCnsModeHifi;
            n_mode[hifi ? 1 : 2]++;
            rq.done = !O.err;
            if (O.err) {
                (hifi ? S.stats.cnsw_hifi_declined : S.stats.cnsw_fast_declined)++;
                continue;
            }
            if (hifi) {
                rq.words.assign(w, w + O.n_words);
                rq.wins.assign(wn, wn + 2 * (size_t)O.n_win);
                rq.len = O.len, rq.lqseq_total_length = O.lqseq_total_length;
                S.stats.cnsw_hifi_jobs++;
                S.stats.cnsw_hifi_regions += O.n_win;
            } else {
                rq.lq_m = O.lq_m, rq.hq_m = O.hq_m, rq.lqseq_total_length = O.lqseq_total_length, rq.len = O.len;
                rq.seq.assign(sq, sq + O.n_bytes);
                S.stats.cnsw_fast_jobs++;
            }
            w += O.n_words, wn += 2 * (size_t)O.n_win, sq += O.n_bytes;
        }
        S.drain();
        if (trace_on())
            fprintf(stderr, "[ndgpu trace] cns_walk %zu walks (batched entry): %zu HiFi, %zu -fast | K21 %.3f ms | %llu words, %llu windows, %llu bytes\n",
                    m, n_mode[1], n_mode[2], S.ms(State::kEvCnswBegin, State::kEvCnswEnd), (unsigned long long)n_words,
                    (unsigned long long)n_wins, (unsigned long long)n_bytes);
        a = b;
    }
}

// ---- K24: the splice, the table of lower-case runs and the SSR trim on the device (nd_splice.h states the rule; DESIGN.md section
// 0a, K24).  run_splice is: pack_splice (the jobs of a launch into four arenas, bounded by a byte budget; what the kernel must
// not compute is marked declined) -> launch_splice_jobs (the arenas up, K24 and its gather) -> fetch_splice (the records, then the
// strings at exact size).  A declined job keeps done == false and the caller takes splice_host.

// Test hook NDGPU_SPLICE_DECLINE=<k>: every k-th job offered to K24 is left to the host (counted over the process).
static bool splice_decline_hook() {
    static const uint64_t k = env_u64("NDGPU_SPLICE_DECLINE", 0);
    static std::atomic<uint64_t> seen{0};
    return k && seen.fetch_add(1) % k == k - 1;
}

size_t DeviceAligner::State::pack_splice(SpliceReq **reqs, size_t a, size_t n, SplicePack &P) {
    constexpr size_t kJobs = 4096, kBytes = (size_t)256 << 20;   // a launch's jobs, and the bytes of its arenas
    constexpr uint64_t kJobCap = (uint64_t)1 << 30;              // words, and words + pseudo-seed bytes, of one job
    P.jobs.clear(), P.regs.clear(), P.words.clear(), P.seeds.clear(), P.ids.clear();
    P.chars = 0;
    size_t b = a;
    for (; b < n && P.jobs.size() < kJobs; b++) {
        SpliceReq &rq = *reqs[b];
        rq.done = false;
        const uint32_t nw = rq.len - rq.lstrip - rq.rstrip;
        uint64_t seed_bytes = 0;
        for (size_t k = 0; k < rq.n_regions; k++)
            if (splice_usable(rq.regions[k].len)) seed_bytes += rq.regions[k].sudoseed_len;
        bool take = (uint64_t)nw + seed_bytes < kJobCap && rq.n_regions < kJobCap;
        for (uint32_t k = 0; take && k < nw; k++) take = (rq.words[rq.lstrip + k] >> 8) <= kSpliceMaxPos;
        if (splice_decline_hook()) take = false;
        if (!take) continue;
        const size_t bytes = (size_t)nw * 5 + 2 * (size_t)seed_bytes + rq.n_regions * sizeof(SpliceRegDev);
        if (!P.jobs.empty() && (P.words.size() * 4 + P.chars + P.seeds.size() + P.regs.size() * sizeof(SpliceRegDev)) + bytes > kBytes) break;
        SpliceJobDev J;
        memset(&J, 0, sizeof(J));
        J.word_off = P.words.size(), J.reg_off = P.regs.size(), J.seed_off = P.seeds.size(), J.out_off = P.chars;
        J.n_words = nw, J.n_regions = (uint32_t)rq.n_regions, J.out_cap = (uint32_t)(nw + seed_bytes), J.hifi = rq.hifi ? 1u : 0u;
        P.words.insert(P.words.end(), rq.words + rq.lstrip, rq.words + rq.lstrip + nw);
        P.regs.resize(P.regs.size() + rq.n_regions);
        SpliceRegDev *R = P.regs.data() + J.reg_off;
        uint32_t reach = 0;
        for (size_t k = rq.n_regions; k-- > 0;) {   // (from the top: reach is a running maximum)
            const SpliceRegion &r = rq.regions[k];
            const bool usable = splice_usable(r.len);
            R[k].start = r.start, R[k].end = r.end, R[k].usable = usable ? 1u : 0u;
            R[k].seed_off = 0, R[k].seed_len = usable ? r.sudoseed_len : 0u;
            if (usable) reach = std::max(reach, std::min(r.end, 1u << 21) + 1u);
            R[k].reach = reach;
        }
        for (size_t k = 0; k < rq.n_regions; k++)
            if (R[k].usable && R[k].seed_len) {
                R[k].seed_off = (uint32_t)(P.seeds.size() - J.seed_off);
                P.seeds.insert(P.seeds.end(), rq.regions[k].sudoseed, rq.regions[k].sudoseed + R[k].seed_len);
            }
        P.chars += J.out_cap;
        P.jobs.push_back(J);
        P.ids.push_back(b);
    }
    return b;
}

void DeviceAligner::State::launch_splice_jobs(const SplicePack &P) {
    hipStream_t st = stream;
    const size_t m = P.jobs.size();
    d_splice_jobs.reserve(m), d_splice_out.reserve(m);
    d_splice_regs.reserve(P.regs.size() + 1), d_splice_words.reserve(P.words.size() + 1), d_splice_seeds.reserve(P.seeds.size() + 1);
    d_splice_chars.reserve(P.chars + 1), d_splice_seq.reserve(P.chars + 1);
    h2d(d_splice_jobs.p, P.jobs.data(), m * sizeof(SpliceJobDev), st);
    h2d(d_splice_regs.p, P.regs.data(), P.regs.size() * sizeof(SpliceRegDev), st);
    h2d(d_splice_words.p, P.words.data(), P.words.size() * sizeof(uint32_t), st);
    h2d(d_splice_seeds.p, P.seeds.data(), P.seeds.size(), st);
    stats.splice_h2d_bytes += m * sizeof(SpliceJobDev) + P.regs.size() * sizeof(SpliceRegDev) + P.words.size() * sizeof(uint32_t) + P.seeds.size();
    mark(kEvSpliceBegin, st);
    NDGPU_DBG(st, "splice: %zu jobs", m);
    launch_splice(d_splice_jobs.p, d_splice_words.p, d_splice_regs.p, d_splice_seeds.p, d_splice_chars.p, d_splice_out.p, d_splice_seq.p,
                  (int)m, st);
    mark(kEvSpliceEnd, st);
    HIP_CHECK(hipGetLastError());
    stats.splice_launches++;
}

void DeviceAligner::State::fetch_splice(SpliceReq **reqs, const SplicePack &P) {
    hipStream_t st = stream;
    const size_t m = P.jobs.size();
    std::vector<SpliceOutDev> outs(m);
    d2h(outs.data(), d_splice_out.p, m * sizeof(SpliceOutDev), st);
    sync_drain(st);
    stats.splice_ms += ms(kEvSpliceBegin, kEvSpliceEnd);
    uint64_t n_bytes = 0;
    for (const SpliceOutDev &O : outs)
        if (!O.err) n_bytes += O.n_bytes;
    reserve_down(n_bytes + 2048, st);
    const char *sq = (const char *)d2h(nullptr, d_splice_seq.p, n_bytes, st);
    HIP_CHECK(hipStreamSynchronize(st));
    stats.splice_d2h_bytes += m * sizeof(SpliceOutDev) + n_bytes;
    for (size_t i = 0; i < m; i++) {
        SpliceReq &rq = *reqs[P.ids[i]];
        const SpliceOutDev &O = outs[i];
        if (O.err) {
            if (O.err != kSpliceErrHook)
                fprintf(stderr, "[ndgpu] splice: a job of %u words left to the host statement (error word %u)\n", P.jobs[i].n_words, O.err);
            continue;
        }
        rq.done = true;
        rq.out_len = O.out_len, rq.lq_m = O.lq_m, rq.hq_m = O.hq_m, rq.lq_total_len = O.lq_total_len, rq.lq_i = O.lq_i;
        rq.clip_s = O.clip_s, rq.clip_e = O.clip_e, rq.code = O.code, rq.trimmed = O.trimmed;
        rq.seq.assign(sq, sq + O.n_bytes);
        sq += O.n_bytes;
        stats.splice_trimmed += O.trimmed;
    }
    drain();
    if (trace_on())
        fprintf(stderr, "[ndgpu trace] splice %zu jobs | K24 %.3f ms | %zu words, %zu regions up, %llu bytes down\n", m,
                ms(kEvSpliceBegin, kEvSpliceEnd), P.words.size(), P.regs.size(), (unsigned long long)n_bytes);
}

void DeviceAligner::run_splice(SpliceReq **reqs, size_t n) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    SplicePack P;
    S.stats.splice_jobs += n;
    size_t taken = 0;
    for (size_t a = 0; a < n;) {
        a = S.pack_splice(reqs, a, n, P);
        if (P.jobs.empty()) continue;
        S.launch_splice_jobs(P);
        S.fetch_splice(reqs, P);
    }
    for (size_t i = 0; i < n; i++) taken += reqs[i]->done ? 1 : 0;
    S.stats.splice_declined += n - taken;
}

void DeviceAligner::run_main(MainPile **mp, size_t np) {
    State &S = *s_;
    uint64_t tp[5] = {wall_ns()};
    const State::Phase phase(S);
    hipStream_t st = S.stream;
    const MainLayout L = S.layout_piles(mp, np);
    std::vector<PileDev> &piles = S.piles;
    const size_t nt = S.tasks.size(), nr = S.reads.size();
    // forward/traceback chunks bounded by the trace budget
    const std::vector<AlignChunk> chunks = S.plan_chunks(S.tasks.data(), nt);
    S.reserve_layout(L, np);
    g_prof.m_prep += (tp[1] = wall_ns()) - tp[0];

    S.h2d(S.d_pool.p, S.pool.data(), S.pool.size() * sizeof(uint32_t), st);
    if (nt) S.h2d(S.d_tasks.p, S.tasks.data(), nt * sizeof(AlnTask), st);
    S.h2d(S.d_reads.p, S.reads.data(), nr * sizeof(ReadDev), st);
    S.h2d(S.d_piles.p, piles.data(), np * sizeof(PileDev), st);
    S.h2d(S.d_read_pile.p, L.read_pile.data(), nr * sizeof(uint32_t), st);
    const CovPlanes cov{S.d_cov.p, S.d_cov.p + (L.col_slots + 1), S.d_cov.p + 2 * (L.col_slots + 1)};
    HIP_CHECK(hipMemsetAsync(cov.cov, 0, 3 * (L.col_slots + 1) * sizeof(uint32_t), st));  // (one fill for the three)
    HIP_CHECK(hipMemsetAsync(S.d_err.p, 0, kErrWords * sizeof(uint32_t), st));
    S.align_main(chunks, np);
    g_prof.m_aln += (tp[2] = wall_ns()) - tp[1];

    S.launch_tags(cov, np);
    S.d2h(piles.data(), S.d_piles.p, np * sizeof(PileDev), st);
    S.sync_drain(st);
    g_prof.m_tags += (tp[3] = wall_ns()) - tp[2];

    const MsaPlan plan = plan_msa(piles);
    S.stats.tags += plan.ents;
    S.stats.cells_msa += plan.cells;
    S.stats.piles += np;
    S.upload_plan(plan);
    bool want_cns = np > 0;   // K20 takes the walks when every pile of the launch asks (the engine asks under NDGPU_CNS_DEVICE=1)
    bool walk_modes = false;  // ... and K21 where one of them is a HiFi or -fast pile (NDGPU_CNS_HIFI=1, NDGPU_CNS_FAST=1)
    for (size_t p = 0; p < np; p++) {
        want_cns = want_cns && mp[p]->want_cns;
        walk_modes = walk_modes || mp[p]->cns_mode != (int)kCnsModeRaw;
        mp[p]->cns_ready = false;
    }
    const CnsPlan cns = !want_cns ? CnsPlan() : walk_modes ? S.plan_cns_walk(plan, mp) : S.plan_cns(plan, mp);
    MsaResult res = S.count_and_score(plan, cov, want_cns ? &cns : nullptr);
    piles.swap(res.piles);
    g_prof.m_msa += (tp[4] = wall_ns()) - tp[3];
    if (res.herr[0]) {
        fprintf(stderr, "[ndgpu] FATAL: a cell of the MSA holds more links than its pile has reads\n");
        abort();
    }
    S.tally_main(plan, L.bad_pile, mp, tp);
    if (want_cns && cns.walk) S.fetch_cns_walk(cns, res, L.bad_pile, mp);
    else if (want_cns) S.fetch_cns(cns, res, L.bad_pile, mp);
    else unpack_paths(piles, res.hpath, L.bad_pile, mp, S.host_threads);
    g_prof.m_post += wall_ns() - tp[4];
}

// ---- POA problems as a batch (K13): lockstep rounds -- round r aligns sequence r of every problem that has one against the
// problem's graph, one launch pair (wave form, workgroup form) per slice of the round that fits the memory plan; between rounds the
// context's host threads thread the routes through the graphs and sort them (poa.cpp).  The workspace -- 6 bytes per cell of
// (X + 1)(Y + 1) -- is charged to the trace budget of the memory plan.  A problem outside the device's limits (a sequence of 0 or
// more than 9,999 bases) or whose round alone exceeds the budget is declined: req.done stays false and the caller takes the host path.
// poa_rounds (below; run_poa's form unless NDGPU_POA_RESIDENT=1 or the caller selects the resident one, K19, further down) is: admit
// (admit_poa) -> per round: export_rows -> per slice: the budget cut (next_poa_slice of nd_lqplan.h) -> stage_poa_slice ->
// launch_poa_slice -> thread_routes -> the consensus of the problems still live.

// Which problems take the device path (PoaProb::live), each with its first sequence as a chain; returns the most sequences of one.
size_t DeviceAligner::State::admit_poa(PoaReq **reqs, size_t n, uint64_t budget, PoaBatch &B) {
    size_t max_seqs = 0;
    stats.poa_jobs += n;
    for (size_t i = 0; i < n; i++) {
        PoaReq &rq = *reqs[i];
        rq.done = false, rq.failed = false;
        if (rq.seqs.size() > (size_t)kPoaMaxSeqs) {
            rq.failed = true;
            continue;
        }
        bool ok = !rq.seqs.empty() && budget > 0;
        for (const std::string &q : rq.seqs) ok = ok && !q.empty() && q.size() <= (size_t)kPoaMaxSeqLen;
        B.probs[i].live = ok;
        if (!ok) continue;
        B.probs[i].g.start(rq.seqs[0].c_str(), rq.seqs[0].size());
        max_seqs = std::max(max_seqs, rq.seqs.size());
    }
    return max_seqs;
}

// Round r of problems ids: every graph as rows, and what the budget cut goes by (load[k] for ids[k]).
void DeviceAligner::State::export_rows(PoaBatch &B, PoaReq **reqs, const std::vector<size_t> &ids, size_t r, std::vector<PoaLoad> &load) {
    poa_each(ids, [&](size_t i) {
        PoaProb &p = B.probs[i];
        p.g.export_rows(p.rows);
        p.cells = (uint64_t)(p.g.rows() + 1) * (uint64_t)(reqs[i]->seqs[r].size() + 1);
    });
    load.resize(ids.size());
    for (size_t k = 0; k < ids.size(); k++) load[k] = PoaLoad{B.probs[ids[k]].cells, (uint64_t)B.probs[ids[k]].g.rows()};
}

// The slice's five tables: jobs, rows, predecessor rows, query bytes, and the ids each kernel form takes (wave jobs, then group jobs).
void DeviceAligner::State::stage_poa_slice(PoaBatch &B, PoaReq **reqs, const std::vector<size_t> &slice, size_t r) {
    const PoaHooks &hk = hooks_of<PoaHooks>();
    B.jobs.clear(), B.rows.clear(), B.preds.clear(), B.qpool.clear(), B.ids.clear();
    B.cells = B.route_words = 0;
    std::vector<uint32_t> ids_group;
    for (size_t i : slice) {
        PoaProb &p = B.probs[i];
        const std::string &q = reqs[i]->seqs[r];
        PoaJobDev J;
        memset(&J, 0, sizeof(J));
        J.X = (uint32_t)p.g.rows(), J.Y = (uint32_t)q.size();
        J.q_off = B.qpool.size(), J.row_off = B.rows.size(), J.pred_off = B.preds.size();
        J.cell_off = B.cells, J.route_off = B.route_words;
        B.cells += p.cells, B.route_words += (uint64_t)J.X + J.Y;
        B.qpool.insert(B.qpool.end(), q.begin(), q.end());
        for (uint32_t x = 0; x < J.X; x++) {
            PoaRowDev rw;
            rw.pred_off = p.rows.pred_off[x];
            rw.n_pred = (uint16_t)(p.rows.pred_off[x + 1] - p.rows.pred_off[x]);
            rw.base = p.rows.base[x], rw.sink = p.rows.sink[x];
            B.rows.push_back(rw);
        }
        B.preds.insert(B.preds.end(), p.rows.preds.begin(), p.rows.preds.end());
        p.job = (uint32_t)B.jobs.size();
        const bool group = hk.form ? hk.form == 2 : J.Y >= hk.group_min;
        (group ? ids_group : B.ids).push_back(p.job);
        B.jobs.push_back(J);
    }
    B.n_wave = B.ids.size();
    B.ids.insert(B.ids.end(), ids_group.begin(), ids_group.end());
}

// Buffers, five uploads, the launch pair in one event bracket, the jobs (their route lengths) and the routes down, one synchronisation.
void DeviceAligner::State::launch_poa_slice(PoaBatch &B, size_t r) {
    hipStream_t st = stream;
    const size_t n_group = B.ids.size() - B.n_wave;
    d_poa_jobs.reserve(B.jobs.size()), d_poa_ids.reserve(B.ids.size()), d_poa_q.reserve(B.qpool.size());
    d_poa_rows.reserve(B.rows.size()), d_poa_preds.reserve(B.preds.size());
    d_poa_s.reserve(B.cells), d_poa_f.reserve(B.cells), d_poa_route.reserve(B.route_words);
    h2d(d_poa_jobs.p, B.jobs.data(), B.jobs.size() * sizeof(PoaJobDev), st);
    h2d(d_poa_ids.p, B.ids.data(), B.ids.size() * sizeof(uint32_t), st);
    h2d(d_poa_q.p, B.qpool.data(), B.qpool.size(), st);
    h2d(d_poa_rows.p, B.rows.data(), B.rows.size() * sizeof(PoaRowDev), st);
    h2d(d_poa_preds.p, B.preds.data(), B.preds.size() * sizeof(uint16_t), st);
    stats.poa_h2d_bytes += B.jobs.size() * sizeof(PoaJobDev) + B.ids.size() * sizeof(uint32_t) + B.qpool.size() +
                           B.rows.size() * sizeof(PoaRowDev) + B.preds.size() * sizeof(uint16_t);
    stats.poa_d2h_bytes += B.jobs.size() * sizeof(PoaJobDev) + B.route_words * sizeof(uint32_t);
    mark(kEvTailBegin, st);
    NDGPU_DBG(st, "poa: round %zu, %zu + %zu jobs, %llu cells", r, B.n_wave, n_group, (unsigned long long)B.cells);
    launch_poa_align(d_poa_jobs.p, d_poa_ids.p, (int)B.n_wave, d_poa_ids.p + B.n_wave, (int)n_group, d_poa_q.p, d_poa_rows.p, d_poa_preds.p,
                     d_poa_s.p, d_poa_f.p, d_poa_route.p, st);
    HIP_CHECK(hipGetLastError());
    mark(kEvTailEnd, st);
    B.routes.resize(B.route_words);
    d2h(B.jobs.data(), d_poa_jobs.p, B.jobs.size() * sizeof(PoaJobDev), st);
    d2h(B.routes.data(), d_poa_route.p, B.route_words * sizeof(uint32_t), st);
    sync_drain(st);
    stats.poa_ms += ms(kEvTailBegin, kEvTailEnd);
    stats.poa_launches += (B.n_wave ? 1 : 0) + (n_group ? 1 : 0);
    stats.poa_cells += B.cells;
}

// Graph growth and the new order, on the host: the slice's routes threaded through their graphs.
void DeviceAligner::State::thread_routes(PoaBatch &B, PoaReq **reqs, const std::vector<size_t> &slice, size_t r) {
    poa_each(slice, [&](size_t i) {
        PoaProb &p = B.probs[i];
        const PoaJobDev &J = B.jobs[p.job];
        const std::string &q = reqs[i]->seqs[r];
        if (J.route_len > J.X + J.Y) {  // (the walk did not reach the origin: cannot happen)
            fprintf(stderr, "[ndgpu] FATAL: POA route of a %u x %u problem did not end\n", J.X, J.Y);
            abort();
        }
        p.g.set_route(B.routes.data() + J.route_off, J.route_len);
        if (!p.g.thread((int)r, q.c_str(), (int)q.size())) p.live = false, reqs[i]->failed = true;
    });
}

void DeviceAligner::run_poa(PoaReq **reqs, size_t n, int form) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    if (form == 1 || (form == 0 && hooks_of<PoaHooks>().resident)) S.poa_resident(reqs, n);
    else S.poa_rounds(reqs, n);
}

void DeviceAligner::State::poa_rounds(PoaReq **reqs, size_t n) {
    State &S = *this;
    const PoaHooks &hk = hooks_of<PoaHooks>();
    const uint64_t budget = hk.budget_set ? hk.budget : (uint64_t)(S.trace_budget_bytes / 6);
    PoaBatch B(n);
    const size_t max_seqs = S.admit_poa(reqs, n, budget, B);
    std::vector<size_t> round_ids, slice, dropped;
    std::vector<PoaLoad> load;
    for (size_t r = 1; r < max_seqs; r++) {
        round_ids.clear();
        for (size_t i = 0; i < n; i++)
            if (B.probs[i].live && reqs[i]->seqs.size() > r) round_ids.push_back(i);
        if (round_ids.empty()) break;
        S.stats.poa_rounds++;
        S.export_rows(B, reqs, round_ids, r, load);
        for (size_t a = 0; a < round_ids.size();) {
            a = next_poa_slice(load, a, budget, slice, dropped);
            for (size_t k : dropped) B.probs[round_ids[k]].live = false;  // (over the budget or the row limit on its own: declined)
            for (size_t &k : slice) k = round_ids[k];
            if (slice.empty()) continue;
            S.stage_poa_slice(B, reqs, slice, r);
            S.launch_poa_slice(B, r);
            S.thread_routes(B, reqs, slice, r);
        }
    }
    round_ids.clear();
    for (size_t i = 0; i < n; i++)
        if (B.probs[i].live) round_ids.push_back(i);
    S.poa_each(round_ids, [&](size_t i) {
        reqs[i]->out = B.probs[i].g.consensus((int)reqs[i]->seqs.size());
        reqs[i]->done = true;
    });
    for (size_t i = 0; i < n; i++)
        if (!reqs[i]->done && !reqs[i]->failed) S.stats.poa_declined++;
}

// ---- POA problems with resident graphs (K19): a problem's graph lives in its arena on the device from its first sequence to its
// consensus string; K13 runs unchanged on the tables K19's rows kernel makes there.  poa_resident (below) is: admit
// (admit_poa_resident: the arenas from the bounds, the rest to poa_rounds) -> start_poa_graphs (every sequence up once, the first ones
// as chains) -> per round poa_resident_round (the budget cut from the X of the round before -> the round's problems up, 16 bytes each
// -> rows kernel -> K13 per launch of the cut -> thread kernel -> 8 bytes a problem down) -> poa_resident_consensus (the strings and
// their lengths down in one copy).  Per round no table goes up and no route comes down.
// The arenas are charged to the budget of the cells: they may take up to half of it (a problem behind that goes to poa_rounds), and
// a round's launches share what the arenas leave.  A problem whose arena plus the cells of its largest round -- at least
// (len_0 + 1)(len_r + 1), since a graph only grows -- exceed the budget does not start here either.

void DeviceAligner::State::admit_poa_resident(PoaReq **reqs, size_t n, uint64_t budget, PoaResident &R, std::vector<PoaReq *> &rest) {
    const uint64_t budget_bytes = budget > UINT64_MAX / 6 ? UINT64_MAX : budget * 6;
    for (size_t i = 0; i < n; i++) {
        PoaReq &rq = *reqs[i];
        rq.done = false, rq.failed = false;
        if (rq.seqs.size() > (size_t)kPoaMaxSeqs) {
            stats.poa_jobs++;   // (poa_rounds counts the ones it is given)
            rq.failed = true;
            continue;
        }
        bool ok = !rq.seqs.empty();
        uint64_t bound = 0, max_len = 0;
        for (const std::string &q : rq.seqs) {
            ok = ok && !q.empty() && q.size() <= (size_t)kPoaMaxSeqLen;
            bound += q.size() + 1;
            if (&q != &rq.seqs[0]) max_len = std::max<uint64_t>(max_len, q.size());
        }
        PoaArena A;
        ok = ok && poa_arena_layout(bound, A);
        if (ok) {
            const uint64_t cells = rq.seqs.size() > 1 ? (uint64_t)(rq.seqs[0].size() + 1) * (max_len + 1) : 0;
            ok = A.bytes + 6 * cells <= budget_bytes && R.arena_bytes + A.bytes <= budget_bytes / 2;
        }
        if (!ok) {
            stats.poa_resident_declined++;
            rest.push_back(&rq);
            continue;
        }
        stats.poa_jobs++;
        PoaGraphDev G;
        memset(&G, 0, sizeof(G));
        G.arena_off = R.arena_bytes, G.out_off = R.out_bytes;
        G.seq_first = (uint32_t)R.seqs.size(), G.n_seq = (uint32_t)rq.seqs.size(), G.bound = (uint32_t)bound;
        R.arena_bytes += A.bytes, R.out_bytes += (bound + 7) & ~(uint64_t)7;
        for (const std::string &q : rq.seqs) {
            R.seqs.push_back(PoaSeqDev{(uint64_t)R.pool.size(), (uint32_t)q.size(), 0});
            R.pool.insert(R.pool.end(), q.begin(), q.end());
            R.pool.push_back('\0');
        }
        R.req.push_back(i), R.graphs.push_back(G), R.live.push_back(1);
        R.xe.push_back(PoaXeDev{(uint32_t)rq.seqs[0].size(), 0});
        R.max_seqs = std::max(R.max_seqs, rq.seqs.size());
    }
}

// Every buffer of the call but the cells, three uploads (problems, sequence table, sequences), the start kernel.
void DeviceAligner::State::start_poa_graphs(PoaResident &R) {
    hipStream_t st = stream;
    const size_t np = R.req.size();
    d_poa_graphs.reserve(np), d_poa_seqs.reserve(R.seqs.size()), d_poa_q.reserve(R.pool.size()), d_poa_jobs.reserve(np);
    d_poa_round.reserve(np), d_poa_ids.reserve(np), d_poa_xe.reserve(np);
    d_poa_out.reserve(((np + 1) & ~(size_t)1) + R.out_bytes / 4), d_poa_arena.reserve(R.arena_bytes / 8);
    h2d(d_poa_graphs.p, R.graphs.data(), np * sizeof(PoaGraphDev), st);
    h2d(d_poa_seqs.p, R.seqs.data(), R.seqs.size() * sizeof(PoaSeqDev), st);
    h2d(d_poa_q.p, R.pool.data(), R.pool.size(), st);
    stats.poa_h2d_bytes += np * sizeof(PoaGraphDev) + R.seqs.size() * sizeof(PoaSeqDev) + R.pool.size();
    mark(kEvPoaRows, st);
    NDGPU_DBG(st, "poa resident: start, %zu problems, %llu arena bytes", np, (unsigned long long)R.arena_bytes);
    launch_poa_graph_start(d_poa_graphs.p, d_poa_xe.p, (unsigned char *)d_poa_arena.p, d_poa_q.p, d_poa_seqs.p, (int)np, st);
    HIP_CHECK(hipGetLastError());
    mark(kEvPoaAlign, st);
    sync_drain(st);
    stats.poa_graph_ms += ms(kEvPoaRows, kEvPoaAlign);
    stats.poa_graph_launches++;
}

// Round r: sequence r of every live problem that has one.
void DeviceAligner::State::poa_resident_round(PoaResident &R, PoaReq **reqs, size_t r, uint64_t budget) {
    const PoaHooks &hk = hooks_of<PoaHooks>();
    hipStream_t st = stream;
    std::vector<size_t> round_ids, slice, dropped;
    std::vector<PoaLoad> load;
    for (size_t p = 0; p < R.req.size(); p++)
        if (R.live[p] && reqs[R.req[p]]->seqs.size() > r) {
            round_ids.push_back(p);
            const uint64_t X = R.xe[p].X;
            load.push_back(PoaLoad{(X + 1) * (uint64_t)(reqs[R.req[p]]->seqs[r].size() + 1), X});
        }
    if (round_ids.empty()) return;
    stats.poa_rounds++;
    // the budget cut, every launch of the round at once (it goes by the loads alone)
    R.round.clear(), R.ids.clear(), R.launches.clear();
    uint64_t max_cells = 0;
    std::vector<uint32_t> ids_group;
    for (size_t a = 0; a < round_ids.size();) {
        a = next_poa_slice(load, a, budget, slice, dropped);
        for (size_t k : dropped) R.live[round_ids[k]] = 0;  // (over what the arenas leave of the budget on its own: it leaves the device path)
        if (slice.empty()) continue;
        PoaResident::Launch L{R.ids.size(), 0, 0, 0};
        ids_group.clear();
        for (size_t k : slice) {
            const size_t p = round_ids[k];
            R.round.push_back(PoaRoundDev{(uint32_t)p, 0, L.cells});
            L.cells += load[k].cells;
            const uint32_t Y = (uint32_t)reqs[R.req[p]]->seqs[r].size();
            const bool group = hk.form ? hk.form == 2 : Y >= hk.group_min;
            (group ? ids_group : R.ids).push_back((uint32_t)p);
        }
        L.n_wave = R.ids.size() - L.first, L.n_group = ids_group.size();
        R.ids.insert(R.ids.end(), ids_group.begin(), ids_group.end());
        R.launches.push_back(L);
        max_cells = std::max(max_cells, L.cells);
    }
    if (R.round.empty()) return;
    d_poa_s.reserve(max_cells), d_poa_f.reserve(max_cells);
    h2d(d_poa_round.p, R.round.data(), R.round.size() * sizeof(PoaRoundDev), st);
    h2d(d_poa_ids.p, R.ids.data(), R.ids.size() * sizeof(uint32_t), st);
    stats.poa_h2d_bytes += R.round.size() * sizeof(PoaRoundDev) + R.ids.size() * sizeof(uint32_t);
    unsigned char *arena = (unsigned char *)d_poa_arena.p;
    mark(kEvPoaRows, st);
    NDGPU_DBG(st, "poa resident: round %zu, rows of %zu problems", r, R.round.size());
    launch_poa_graph_rows(d_poa_graphs.p, d_poa_round.p, (int)R.round.size(), (uint32_t)r, arena, d_poa_seqs.p, d_poa_jobs.p, st);
    mark(kEvPoaAlign, st);
    uint64_t cells = 0;
    for (const PoaResident::Launch &L : R.launches) {  // (one after the other on the stream: they share the cells)
        NDGPU_DBG(st, "poa resident: round %zu, %zu + %zu jobs, %llu cells", r, L.n_wave, L.n_group, (unsigned long long)L.cells);
        launch_poa_align(d_poa_jobs.p, d_poa_ids.p + L.first, (int)L.n_wave, d_poa_ids.p + L.first + L.n_wave, (int)L.n_group, d_poa_q.p,
                         (const PoaRowDev *)arena, (const uint16_t *)arena, d_poa_s.p, d_poa_f.p, (uint32_t *)arena, st);
        stats.poa_launches += (L.n_wave ? 1 : 0) + (L.n_group ? 1 : 0);
        cells += L.cells;
    }
    mark(kEvPoaThread, st);
    NDGPU_DBG(st, "poa resident: round %zu, thread", r);
    launch_poa_graph_thread(d_poa_graphs.p, d_poa_xe.p, d_poa_round.p, (int)R.round.size(), (uint32_t)r, arena, d_poa_q.p, d_poa_seqs.p,
                            d_poa_jobs.p, st);
    HIP_CHECK(hipGetLastError());
    mark(kEvPoaEnd, st);
    d2h(R.xe.data(), d_poa_xe.p, R.xe.size() * sizeof(PoaXeDev), st);
    sync_drain(st);
    stats.poa_d2h_bytes += R.xe.size() * sizeof(PoaXeDev);
    stats.poa_cells += cells;
    stats.poa_graph_launches += 2;
    const double g_ms = ms(kEvPoaRows, kEvPoaAlign) + ms(kEvPoaThread, kEvPoaEnd), a_ms = ms(kEvPoaAlign, kEvPoaThread);
    stats.poa_graph_ms += g_ms, stats.poa_ms += a_ms;
    size_t gone = 0;
    for (const PoaRoundDev &d : R.round)
        if (R.xe[d.prob].err) R.live[d.prob] = 0, gone++;   // a capacity or a trip bound reached: the host path computes it
    if (trace_on())
        fprintf(stderr, "[ndgpu trace] poa resident round %zu: %zu problems in %zu launches, %llu cells, graph %.3f ms, align %.3f ms, %zu left the path\n",
                r, R.round.size(), R.launches.size(), (unsigned long long)cells, g_ms, a_ms, gone);
}

// The heaviest paths of the problems still live; strings and lengths down in one copy.
void DeviceAligner::State::poa_resident_consensus(PoaResident &R, PoaReq **reqs) {
    hipStream_t st = stream;
    const size_t np = R.req.size();
    R.ids.clear();
    for (size_t p = 0; p < np; p++)
        if (R.live[p]) R.ids.push_back((uint32_t)p);
    if (R.ids.empty()) return;
    const size_t len_words = (np + 1) & ~(size_t)1;   // the lengths, then the strings from a multiple of 8 bytes on
    h2d(d_poa_ids.p, R.ids.data(), R.ids.size() * sizeof(uint32_t), st);
    stats.poa_h2d_bytes += R.ids.size() * sizeof(uint32_t);
    mark(kEvPoaRows, st);
    NDGPU_DBG(st, "poa resident: consensus of %zu problems", R.ids.size());
    launch_poa_graph_consensus(d_poa_graphs.p, d_poa_ids.p, (int)R.ids.size(), (unsigned char *)d_poa_arena.p, (char *)(d_poa_out.p + len_words),
                               d_poa_out.p, st);
    HIP_CHECK(hipGetLastError());
    mark(kEvPoaAlign, st);
    std::vector<uint32_t> out(len_words + R.out_bytes / 4);
    d2h(out.data(), d_poa_out.p, out.size() * sizeof(uint32_t), st);
    sync_drain(st);
    stats.poa_d2h_bytes += out.size() * sizeof(uint32_t);
    stats.poa_graph_ms += ms(kEvPoaRows, kEvPoaAlign);
    stats.poa_graph_launches++;
    const char *str = (const char *)(out.data() + len_words);
    for (uint32_t p : R.ids) {
        const uint32_t len = out[p];
        if (len > R.graphs[p].bound) continue;   // (0xffffffff: the kernel gave the problem up)
        PoaReq &rq = *reqs[R.req[p]];
        rq.out.assign(str + R.graphs[p].out_off, len);
        rq.done = true;
        stats.poa_resident_jobs++;
    }
}

void DeviceAligner::State::poa_resident(PoaReq **reqs, size_t n) {
    const PoaHooks &hk = hooks_of<PoaHooks>();
    const uint64_t budget = hk.budget_set ? hk.budget : (uint64_t)(trace_budget_bytes / 6);
    PoaResident R;
    std::vector<PoaReq *> rest;
    admit_poa_resident(reqs, n, budget, R, rest);
    if (!R.req.empty()) {
        start_poa_graphs(R);
        const uint64_t left = budget - (R.arena_bytes + 5) / 6;   // (the arenas took at most half)
        for (size_t r = 1; r < R.max_seqs; r++) poa_resident_round(R, reqs, r, left);
        poa_resident_consensus(R, reqs);
        for (size_t p = 0; p < R.req.size(); p++)
            if (!reqs[R.req[p]]->done) stats.poa_resident_declined++, stats.poa_declined++;
    }
    if (!rest.empty()) poa_rounds(rest.data(), rest.size());
}

// The ranking K14 left in a region's record (ranked != 0), for whoever asked: run_rank's problems, run_extract's regions.
template <typename Tail>
static void read_ranking(const RegionDev &g, uint8_t (&order)[40], uint16_t (&kscore)[40], Tail &tail) {
    memcpy(order, g.rank_order, sizeof(order));
    memcpy(kscore, g.rank_kscore, sizeof(kscore));
    tail = g.rank_tail;
}

// ---- the 8-mer ranking as a batch (K14): the problems' sequences go up as one pool, laid out as K11 leaves a region's candidates
// (RegionDev::cand_off / cand_len), one launch per slice of at most kRankSliceBytes, the records come back in one copy.
void DeviceAligner::run_rank(RankReq *reqs, size_t n) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    hipStream_t st = S.stream;
    constexpr size_t kRankSliceBytes = (size_t)256 << 20, kRankSliceJobs = 1 << 20;
    std::vector<RegionDev> regs;
    std::vector<char> pool;
    for (size_t a = 0; a < n;) {
        regs.clear(), pool.clear();
        size_t b = a;
        for (; b < n && b - a < kRankSliceJobs; b++) {
            const RankReq &rq = reqs[b];
            size_t bytes = 0;
            for (int k = 0; k < rq.n; k++) bytes += rq.len[k];
            if (b > a && pool.size() + bytes > kRankSliceBytes) break;
            RegionDev g;
            memset(&g, 0, sizeof(g));
            g.n_ok = (uint32_t)rq.n;
            g.want_rank = 1;
            for (int k = 0; k < rq.n; k++) {
                g.cand_off[k] = (uint32_t)pool.size();
                g.cand_len[k] = rq.len[k];
                pool.insert(pool.end(), rq.seqs[k], rq.seqs[k] + rq.len[k]);
            }
            regs.push_back(g);
        }
        S.d_regions.reserve(regs.size());
        S.d_strpool.reserve(pool.size() + 1);
        S.h2d(S.d_regions.p, regs.data(), regs.size() * sizeof(RegionDev), st);
        S.h2d(S.d_strpool.p, pool.data(), pool.size(), st);
        S.mark(State::kEvTailBegin, st);
        NDGPU_DBG(st, "rank: %zu problems, %zu bytes", regs.size(), pool.size());
        launch_lq_rank(S.d_regions.p, S.d_strpool.p, (unsigned long long)pool.size(), 1u, (int)regs.size(), st);
        HIP_CHECK(hipGetLastError());
        S.mark(State::kEvTailEnd, st);
        S.d2h(regs.data(), S.d_regions.p, regs.size() * sizeof(RegionDev), st);
        S.sync_drain(st);
        S.stats.rank_ms += S.ms(State::kEvTailBegin, State::kEvTailEnd);
        S.stats.rank_launches++;
        for (size_t i = a; i < b; i++) {
            const RegionDev &g = regs[i - a];
            if (!g.ranked) {  // (cannot happen: every problem has 1..40 sequences inside the pool)
                fprintf(stderr, "[ndgpu] FATAL: the ranking kernel left a problem of %d sequences\n", reqs[i].n);
                abort();
            }
            read_ranking(g, reqs[i].order, reqs[i].kscore, reqs[i].tail);
            S.stats.rank_jobs++;
            S.stats.rank_tail += g.rank_tail;
        }
        a = b;
    }
}

// ---- candidate extraction (K11) of the piles run_main left on the device, with the ranking of their regions (K14) behind it where
// a pile asks for it.  run_extract (below) is: regions_of -> extract_into_pool -> the NDGPU_TRACE line -> fill_regions.

// Every region of every pile as a device record, in the piles' order.
static std::vector<RegionDev> regions_of(ExtractPile **ep, size_t n, bool offer_rank) {
    std::vector<RegionDev> regs;
    for (size_t i = 0; i < n; i++)
        for (RegionReq &r : ep[i]->regions) {
            RegionDev g;
            memset(&g, 0, sizeof(g));
            g.pile = (uint32_t)ep[i]->slot;
            g.start = r.start, g.end = r.end, g.max_len = r.max_len;
            g.max_len0 = r.max_len0 ? r.max_len0 : r.max_len;
            g.want_rank = offer_rank && ep[i]->rank ? 1 : 0;
            r.ranked = false;
            regs.push_back(g);
        }
    return regs;
}

// K11 (and K14 behind it, if rank) until the string pool held everything: leaves the records in regs and the strings in hstr, returns
// the number of launches that came back short.  First guess of the pool: 64 MB, or less when the regions cannot
// produce that much (<= 40 candidates of <= max_len characters each) -- or NDGPU_EXTRACT_POOL; what the context holds already wins if
// larger.  The kernel reports what it needed and a pool that was too small is retaken at the exact size.
unsigned DeviceAligner::State::extract_into_pool(std::vector<RegionDev> &regs, bool rank, std::vector<char> &hstr) {
    hipStream_t st = stream;
    d_regions.reserve(regs.size());
    d_cursor.reserve(2);
    size_t bound = (size_t)1 << 20;
    for (const RegionDev &g : regs) bound += (size_t)40 * ((size_t)g.max_len + 64);
    const ExtractHooks &hk = hooks_of<ExtractHooks>();
    size_t cap = std::max<size_t>(d_strpool.cap, hk.pool_set ? hk.pool : std::min<size_t>((size_t)64 << 20, bound));
    for (unsigned retaken = 0;; retaken++) {
        d_strpool.reserve(cap);
        cap = d_strpool.cap;
        h2d(d_regions.p, regs.data(), regs.size() * sizeof(RegionDev), st);
        HIP_CHECK(hipMemsetAsync(d_cursor.p, 0, sizeof(unsigned long long), st));
        mark(kEvTailBegin, st);
        NDGPU_DBG(st, "extract: %zu regions", regs.size());
        launch_extract(d_piles.p, d_reads.p, d_acc.p, d_tags.p, d_colidx.p, d_regions.p, d_strpool.p, d_cursor.p, (unsigned long long)cap,
                       (int)regs.size(), st);
        mark(kEvTailEnd, st);
        // the ranking of the regions with five or more candidates (fewer: the engine drops the region), on the strings where K11
        // left them; with a pool that was too small K14 leaves the regions it cannot read and runs again with K11
        if (rank) {
            launch_lq_rank(d_regions.p, d_strpool.p, (unsigned long long)cap, 5u, (int)regs.size(), st);
            mark(kEvExtractRanked, st);
        }
        unsigned long long used = 0;
        d2h(&used, d_cursor.p, sizeof(used), st);
        sync_drain(st);
        stats.extract_ms += ms(kEvTailBegin, kEvTailEnd);
        if (rank) {
            stats.rank_ms += ms(kEvTailEnd, kEvExtractRanked);
            stats.rank_launches++;
        }
        if (used <= cap) {
            hstr.resize((size_t)used + 1);
            d2h(regs.data(), d_regions.p, regs.size() * sizeof(RegionDev), st);
            if (used) d2h(hstr.data(), d_strpool.p, (size_t)used, st);
            sync_drain(st);
            return retaken;
        }
        cap = (size_t)used + ((size_t)16 << 20);  // pool too small: rerun with the exact size
    }
}

// ---- the phasing and ranking of HiFi candidates (K22)

// Test hook NDGPU_PHASE_DECLINE=<k>: every k-th pile offered to K22 is left to the host rule (counted over the process).
static bool phase_decline_hook() {
    static const uint64_t k = env_u64("NDGPU_PHASE_DECLINE", 0);
    static std::atomic<uint64_t> seen{0};
    return k && seen.fetch_add(1) % k == k - 1;
}

// K22 over the region records and the string pool as they stand on the device (behind K11 in run_extract, behind run_phase's upload):
// pp names the piles that ask and their regions among the launch's n_regions.  The piles' records and the regions' records come back
// in two exact-size copies; a pile with an error word is counted as declined, its regions' records mean nothing.
void DeviceAligner::State::phase_on_pool(std::vector<PhasePileDev> &pp, std::vector<PhaseRegionDev> &recs, size_t n_regions, size_t pool_cap,
                                         const char *who) {
    hipStream_t st = stream;
    d_phase_piles.reserve(pp.size());
    d_phase_out.reserve(n_regions);
    d_phase_work.reserve(n_regions * kPhaseWorkWords);
    h2d(d_phase_piles.p, pp.data(), pp.size() * sizeof(PhasePileDev), st);
    HIP_CHECK(hipMemsetAsync(d_phase_out.p, 0, n_regions * sizeof(PhaseRegionDev), st));
    mark(kEvPhaseBegin, st);
    NDGPU_DBG(st, "phase: %zu piles, %zu regions", pp.size(), n_regions);
    launch_hifi_phase(d_regions.p, d_strpool.p, (unsigned long long)pool_cap, d_phase_piles.p, (int)pp.size(), d_phase_out.p, d_phase_work.p,
                      (int)n_regions, st);
    HIP_CHECK(hipGetLastError());
    mark(kEvPhaseEnd, st);
    recs.resize(n_regions);
    d2h(pp.data(), d_phase_piles.p, pp.size() * sizeof(PhasePileDev), st);
    d2h(recs.data(), d_phase_out.p, n_regions * sizeof(PhaseRegionDev), st);
    sync_drain(st);
    const double t_ms = ms(kEvPhaseBegin, kEvPhaseEnd);
    stats.phase_ms += t_ms;
    stats.phase_launches++;
    stats.phase_d2h_records += pp.size() * sizeof(PhasePileDev) + n_regions * sizeof(PhaseRegionDev);
    uint64_t n_done = 0, n_decl = 0, n_kind[4] = {0, 0, 0, 0}, n_tail = 0, n_pass2 = 0, n_lower = 0;
    for (const PhasePileDev &P : pp) {
        if (P.err) {
            n_decl++;
            for (int b = 0; b < 5; b++) stats.phase_declined[b] += (P.err >> b) & 1u;
            if (P.err != kPhaseErrHook)
                fprintf(stderr, "[ndgpu] hifi_phase: a pile of %u regions, %u reads left to the host rule (error word %u)\n", P.n_regions,
                        P.n_aligned, P.err);
            continue;
        }
        n_done++;
        n_pass2 += P.pass2;
        for (uint32_t r = 0; r < P.n_regions; r++) {
            const PhaseRegionDev &o = recs[P.first_region + r];
            if (o.kind > kPhaseRanked) {  // (cannot happen: every region of a pile the kernel finished has its record)
                fprintf(stderr, "[ndgpu] FATAL: the phasing kernel left a region unfinished (kind %u)\n", (unsigned)o.kind);
                abort();
            }
            n_kind[o.kind]++;
            n_tail += o.tail;
            n_lower += o.kind == kPhaseSeed ? o.lower : 0;
        }
    }
    stats.phase_piles += n_done, stats.phase_pass2 += n_pass2, stats.phase_tail += n_tail, stats.phase_lower += n_lower;
    for (int k = 0; k < 4; k++) stats.phase_kind[k] += n_kind[k], stats.phase_regions += n_kind[k];
    if (trace_on())
        fprintf(stderr, "[ndgpu trace] hifi_phase %zu piles (%s): %zu regions | K22 %.3f ms | empty %llu, dropped %llu, seed %llu, ranked %llu "
                "(%llu tail passes), %llu second passes, %llu declined\n", pp.size(), who, n_regions, t_ms, (unsigned long long)n_kind[0],
                (unsigned long long)n_kind[1], (unsigned long long)n_kind[2], (unsigned long long)n_kind[3], (unsigned long long)n_tail,
                (unsigned long long)n_pass2, (unsigned long long)n_decl);
}

// The batched entry's piles: the candidates go up as one pool, laid out as K11 leaves them (RegionDev::n_ok / cand_off / cand_len /
// cand_rank), one launch per slice; a declined pile keeps done == false.
void DeviceAligner::run_phase(PhaseReq *reqs, size_t n) {
    if (n == 0) return;
    State &S = *s_;
    const State::Phase phase(S);
    hipStream_t st = S.stream;
    constexpr size_t kSliceBytes = (size_t)256 << 20, kSliceRegions = 1 << 18;
    std::vector<RegionDev> regs;
    std::vector<char> pool;
    std::vector<PhasePileDev> pp;
    std::vector<PhaseRegionDev> recs;
    for (size_t a = 0; a < n;) {
        regs.clear(), pool.clear(), pp.clear();
        size_t b = a;
        for (; b < n; b++) {
            const PhaseReq &rq = reqs[b];
            size_t bytes = 0;
            for (size_t r = 0; r < rq.n_regions; r++)
                for (int c = 0; c < rq.regions[r].n_cand; c++) bytes += rq.regions[r].len[c];
            if (b > a && (pool.size() + bytes > kSliceBytes || regs.size() + rq.n_regions > kSliceRegions)) break;
            PhasePileDev P;
            memset(&P, 0, sizeof(P));
            P.first_region = (uint32_t)regs.size(), P.n_regions = (uint32_t)rq.n_regions, P.n_aligned = rq.n_aligned;
            P.decline = phase_decline_hook() ? 1u : 0u;
            pp.push_back(P);
            for (size_t r = 0; r < rq.n_regions; r++) {
                const PhaseRegionIn &in = rq.regions[r];
                RegionDev g;
                memset(&g, 0, sizeof(g));
                g.pile = (uint32_t)(b - a);
                g.start = in.start, g.end = in.end;
                g.n_ok = (uint32_t)in.n_cand;
                for (int c = 0; c < in.n_cand; c++) {
                    g.cand_off[c] = (uint32_t)pool.size();
                    g.cand_len[c] = in.len[c];
                    g.cand_rank[c] = in.src[c];
                    pool.insert(pool.end(), in.seq[c], in.seq[c] + in.len[c]);
                }
                regs.push_back(g);
            }
        }
        if (!regs.empty()) {
            S.d_regions.reserve(regs.size());
            S.d_strpool.reserve(pool.size() + 1);
            S.h2d(S.d_regions.p, regs.data(), regs.size() * sizeof(RegionDev), st);
            S.h2d(S.d_strpool.p, pool.data(), pool.size(), st);
            S.phase_on_pool(pp, recs, regs.size(), pool.size(), "batched entry");
        }
        for (size_t i = a; i < b; i++) {
            PhaseReq &rq = reqs[i];
            const PhasePileDev &P = pp[i - a];
            if (regs.empty()) {   // (piles without regions: nothing to phase)
                rq.done = true;
                continue;
            }
            rq.done = !P.err;
            if (!rq.done) continue;
            rq.pile.has_heter = (uint8_t)(P.has_heter != 0u), rq.pile.pass2 = (uint8_t)(P.pass2 != 0u);
            for (size_t r = 0; r < rq.n_regions; r++) rq.out[r] = recs[P.first_region + r];
        }
        a = b;
    }
}

// The records and their strings into the callers' regions: piles dealt to the context's host threads.
static void fill_regions(ExtractPile **ep, size_t n, const std::vector<RegionDev> &regs, const std::vector<char> &hstr, int host_threads,
                         const std::vector<PhaseRegionDev> &phase_recs, const std::vector<uint8_t> &pile_phased) {
    std::vector<size_t> first(n + 1, 0);
    for (size_t i = 0; i < n; i++) first[i + 1] = first[i] + ep[i]->regions.size();
    host_ranges(n, n < 32 || host_threads <= 1, host_threads, n / 8, [&](size_t a, size_t b) {
        for (size_t i = a; i < b; i++) {
            size_t k = first[i];
            for (RegionReq &r : ep[i]->regions) {
                r.phased = pile_phased[i] != 0;
                if (r.phased) r.phase = phase_recs[k];
                const RegionDev &g = regs[k++];
                r.n_large = g.n_large;
                r.ranked = g.ranked != 0;
                if (r.ranked) read_ranking(g, r.rank_order, r.rank_kscore, r.rank_tail);
                r.cands.resize(g.n_ok);
                r.cand_rank.resize(g.n_ok);
                for (uint32_t c = 0; c < g.n_ok; c++) {
                    r.cands[c].assign(hstr.data() + g.cand_off[c], g.cand_len[c]);
                    r.cand_rank[c] = g.cand_rank[c];
                }
            }
        }
    });
}

void DeviceAligner::run_extract(ExtractPile **ep, size_t n, bool offer_rank) {
    State &S = *s_;
    const State::Phase phase(S);
    std::vector<RegionDev> regs = regions_of(ep, n, offer_rank);
    if (regs.empty()) return;
    // K14 behind K11: some pile of this launch takes a ranking
    const bool rank = std::any_of(regs.begin(), regs.end(), [](const RegionDev &g) { return g.want_rank != 0; });
    std::vector<char> hstr;
    const unsigned retaken = S.extract_into_pool(regs, rank, hstr);
    uint64_t n_ranked = 0, n_tail = 0;
    for (const RegionDev &g : regs) n_ranked += g.ranked ? 1 : 0, n_tail += g.ranked ? g.rank_tail : 0;
    S.stats.rank_jobs += n_ranked, S.stats.rank_tail += n_tail;
    if (trace_on()) {
        char again[48] = "";  // (only a pool that was retaken says so: NDGPU_EXTRACT_POOL, or a bound beyond 64 MB)
        if (retaken) snprintf(again, sizeof(again), ", pool retaken %u", retaken);
        fprintf(stderr, "[ndgpu] extract: %zu regions, %llu ranked on the device, %llu tail passes%s\n", regs.size(),
                (unsigned long long)n_ranked, (unsigned long long)n_tail, again);
    }
    // K22 behind K11 (and K14): the HiFi piles of this launch that ask, on the records and the strings where K11 left them.  Every
    // string still comes down: the engine's selection loop, its POA hand-over and the low-quality-region rounds read them.
    std::vector<PhaseRegionDev> phase_recs;
    std::vector<uint8_t> pile_phased(n, 0);
    if (std::any_of(ep, ep + n, [](const ExtractPile *p) { return p->phase && !p->regions.empty(); })) {
        std::vector<PhasePileDev> pp;
        std::vector<size_t> owner;
        size_t first = 0;
        for (size_t i = 0; i < n; first += ep[i]->regions.size(), i++) {
            if (!ep[i]->phase || ep[i]->regions.empty()) continue;
            PhasePileDev P;
            memset(&P, 0, sizeof(P));
            P.first_region = (uint32_t)first, P.n_regions = (uint32_t)ep[i]->regions.size(), P.n_aligned = ep[i]->n_aligned;
            P.decline = phase_decline_hook() ? 1u : 0u;
            pp.push_back(P);
            owner.push_back(i);
        }
        S.phase_on_pool(pp, phase_recs, regs.size(), hstr.size() - 1, "behind extract");   // (the pool as far as K11 wrote it)
        for (size_t k = 0; k < pp.size(); k++) pile_phased[owner[k]] = pp[k].err ? 0 : 1;
        S.stats.phase_d2h_strings += hstr.size() - 1;
    }
    fill_regions(ep, n, regs, hstr, S.host_threads, phase_recs, pile_phased);
}

}  // namespace ndgpu
