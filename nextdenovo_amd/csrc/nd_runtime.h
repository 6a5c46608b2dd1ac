// Device runtime interface (one instance per process, lazily created on the first
// alignment so that a fork()ed worker pool -- lib/nextcorrect.py:232 -- initialises
// HIP in the child, never in the parent).
#pragma once

#include <cstddef>
#include <cstdint>
#include <cstdlib>
#include <string>
#include <vector>

#include "nd_host.h"

namespace ndgpu {

struct RuntimeStats {
    uint64_t tasks = 0;            // alignments executed
    uint64_t wide_tasks = 0;       // of which needed the HBM-ring kernel
    uint64_t cells = 0;            // (d,k) cells evaluated
    uint64_t d_steps = 0;          // edit steps executed
    uint64_t trace_bits = 0;       // 1-bit move records of alignments that finished
    uint64_t columns = 0;          // alignment columns produced
    uint64_t pool_bases = 0;       // bases packed + uploaded per batch (0 for DB-resident sequences)
    uint64_t seq_bases = 0;        // sum of q_len + t_len over all alignments (operand bases)
    uint32_t max_band = 0;
    uint32_t forward_launches = 0;
    double forward_ms = 0;         // HIP-event time of the forward kernel launches
    double traceback_ms = 0;       // K8a
    double tags_ms = 0;            // K8s + accept + K8b + column scan
    double links_ms = 0;           // K9
    double score_ms = 0;           // K10 (+ backtrack)
    double extract_ms = 0;         // K11
    uint64_t piles = 0;            // piles through the device main phase
    uint64_t tags = 0;             // alignment tags generated on the device
    uint64_t cells_msa = 0;        // MSA cells
    uint64_t path_items = 0;
    uint64_t links = 0;            // distinct MSA links
    uint64_t score_launches = 0;
    double backtrack_ms = 0;
    uint64_t score_segments = 0;   // K10 segments scored
    uint64_t score_repairs = 0;    // of which the stitch kernel scored again (a boundary check failed)
    uint64_t score_slow_piles = 0; // piles that went through the int64 HBM-resident scoring kernel
    uint64_t trace_words = 0;      // 64-bit words of trace records the register-path forward kernel wrote
    uint64_t lq_rounds = 0;        // low-quality-region rounds (pile x round) handed to K12
    uint64_t lq_declined = 0;      // of which the kernel declined (host path took them)
    double lq_ms = 0;              // K12
    uint64_t allocs = 0;           // device / pinned buffers (re)allocated while batches were running, since the last reset
    double alloc_ms = 0;           // wall time of those calls (an allocation in the middle of a step stalls every context)
    uint64_t level_allocs = 0;     // the same between batches (level_buffers: nothing in flight)
    double level_ms = 0;
    // per-kernel launch counts and the algorithmic units of K8a / K12, for the roofline entries of bench.py
    uint64_t traceback_launches = 0;  // K8a launches (main phase + low-quality-region rounds)
    uint64_t lq_launches = 0;         // K12 launches
    uint64_t lq_columns = 0;          // columns of the linked pseudo-seeds K12 walked
    uint64_t lq_aln_columns = 0;      // alignment columns (2-bit kinds) K12 read
    uint64_t lq_bases = 0;            // candidate bases (2-bit) K12 read
    uint64_t lq_out = 0;              // consensus characters K12 wrote
    uint64_t lq_jobs = 0;             // K12 jobs (runs of regions scored from a speculative start)
    uint64_t lq_repairs = 0;          // of which the stitch kernel scored again (failed boundary check)
    uint64_t tb_tasks = 0;            // alignments whose traceback ran in segments
    uint64_t tb_walkers = 0;          // walkers (segments) of those
    uint64_t tb_fallbacks = 0;        // of the alignments: refused by the stitch, walked again by the one-lane kernel
    // POA problems as device batches (K13)
    uint64_t poa_jobs = 0;            // problems offered to run_poa
    uint64_t poa_declined = 0;        // of which declined (outside the device's limits or the memory plan): the host path took them
    uint64_t poa_rounds = 0;          // lockstep rounds (sequence r of every problem that has one)
    uint64_t poa_launches = 0;        // kernel launches
    uint64_t poa_cells = 0;           // (X + 1)(Y + 1) cells filled
    double poa_ms = 0;                // HIP-event time of K13
    // the 8-mer ranking of low-quality-region candidates on the device (K14)
    uint64_t rank_jobs = 0;           // regions / problems ranked
    uint64_t rank_tail = 0;           // of which took the tail pass
    uint64_t rank_launches = 0;       // kernel launches
    double rank_ms = 0;               // HIP-event time of K14
    // batched global alignment with the CIGARs built on the device (K15)
    uint64_t aln_batch_jobs = 0;      // jobs through align_batch_runs
    uint64_t aln_batch_launches = 0;  // launches of K15's emit pass (one per chunk that has a run)
    uint64_t aln_batch_runs = 0;      // runs written
    double aln_batch_ms = 0;          // HIP-event time of K15 (count + emit)
    // resident POA graphs (K19); the two byte counts are kept by both forms of run_poa
    uint64_t poa_resident_jobs = 0;      // problems that finished on the resident path
    uint64_t poa_resident_declined = 0;  // offered to it and not finished there: over the node bound or the budget, or a loop bound hit
    uint64_t poa_graph_launches = 0;     // launches of K19's four kernels
    double poa_graph_ms = 0;             // their HIP-event time
    uint64_t poa_h2d_bytes = 0;          // what run_poa sent to the device
    uint64_t poa_d2h_bytes = 0;          // and what it brought back
    // consensus words and low-quality windows of the walk on the device (K20)
    uint64_t cns_jobs = 0;               // walks K20 finished (run_main's piles, run_cns's jobs)
    uint64_t cns_declined = 0;           // walks it left to the host routine (an error word, or the hook NDGPU_CNS_DECLINE)
    uint64_t cns_launches = 0;           // launches of K20 (each with its gather)
    uint64_t cns_regions = 0;            // windows it emitted
    double cns_ms = 0;                   // HIP-event time of K20 and its gather
    uint64_t cns_d2h_bytes = 0;          // result records, dense words and windows brought back
    uint64_t walk_d2h_bytes = 0;         // bytes of the walks (PathItems) run_main brought back, with or without K20
    // the HiFi and -fast forms of that loop on the device (K21; ndgpu_cns_mode_stats)
    uint64_t cnsw_hifi_jobs = 0;         // HiFi walks K21 finished (run_main's piles, run_cns_walk's jobs)
    uint64_t cnsw_hifi_declined = 0;     // ... and left to the host routine
    uint64_t cnsw_hifi_regions = 0;      // windows it emitted
    uint64_t cnsw_fast_jobs = 0;         // -fast walks it finished
    uint64_t cnsw_fast_declined = 0;
    uint64_t cnsw_launches = 0;          // launches of K21 (each with its gather)
    double cnsw_ms = 0;                  // their HIP-event time
    uint64_t cnsw_d2h_bytes = 0;         // result records, dense words, windows and strings brought back
    // the phasing and ranking of HiFi candidates on the device (K22; ndgpu_phase_stats)
    uint64_t phase_piles = 0;            // piles K22 finished (run_extract's piles, run_phase's jobs)
    uint64_t phase_regions = 0;          // their regions ...
    uint64_t phase_kind[4] = {0, 0, 0, 0};  // ... by kind (kPhaseEmpty, kPhaseDropped, kPhaseSeed, kPhaseRanked)
    uint64_t phase_pass2 = 0;            // piles whose second pass ran
    uint64_t phase_tail = 0;             // ranked regions that took the tail pass
    uint64_t phase_lower = 0;            // seed regions whose pseudo-seed goes to lower case
    uint64_t phase_declined[5] = {0, 0, 0, 0, 0};  // piles left to the host rule, by kPhaseErr* bit: reads, regions, pool, hook, source
    uint64_t phase_launches = 0;         // launches of K22 (its two kernels)
    double phase_ms = 0;                 // their HIP-event time
    uint64_t phase_d2h_records = 0;      // bytes of pile and region records brought back
    uint64_t phase_d2h_strings = 0;      // bytes of candidate strings brought back beside them (run_extract)
    // the splice, its table of lower-case runs and the SSR trim on the device (K24; ndgpu_get_splice_stats)
    uint64_t splice_jobs = 0;            // jobs offered to run_splice
    uint64_t splice_declined = 0;        // ... of which the host statement took (arena caps, a position outside the words' range, the hook)
    uint64_t splice_launches = 0;        // launches of K24 (each with its gather)
    uint64_t splice_h2d_bytes = 0;       // job and region records, words and pseudo-seed bytes sent up
    uint64_t splice_d2h_bytes = 0;       // result records and result strings brought back
    uint64_t splice_trimmed = 0;         // jobs whose gate let the SSR trim run
    double splice_ms = 0;                // K24's HIP-event time
};

// One pile of the batched entry ndgpu_hifi_phase_batch (DeviceAligner::run_phase): what hifi_phase_host (nd_phase.h) returns for it.
struct PhaseReq {
    unsigned n_aligned = 0;
    const PhaseRegionIn *regions = nullptr;
    size_t n_regions = 0;
    PhaseRecord *out = nullptr;            // n_regions records
    PhasePileOut pile;
    bool done = false;                     // false: declined, the host rule takes the pile
};

// One walk of the batched entry ndgpu_cns_walk_batch in mode 1 (HiFi: cns_kmer_host of nd_cns.h) or 2 (-fast: cns_fast_host).
struct CnsWalkReq {
    const PathStep *steps = nullptr;
    size_t n = 0;
    int min_cov = 0;
    int mode = 1;
    const uint8_t *seed_codes = nullptr;   // mode 1: the seed's codes (cns_base_code), seed_len of them
    size_t seed_len = 0;
    bool done = false;
    std::vector<uint32_t> words, wins;     // mode 1
    uint32_t len = 0;                      // mode 1: consensus bases; mode 2: characters emitted
    uint32_t lqseq_total_length = 0;       // mode 2: lq_total_len of the result
    uint32_t lq_m = 0, hq_m = 0;           // mode 2
    std::string seq;                       // mode 2: [lq_m, hq_m) reversed
};

// One walk of the batched entry ndgpu_cns_windows_batch (DeviceAligner::run_cns): what cns_windows_host (nd_cns.h) returns for it.
struct CnsReq {
    const PathStep *steps = nullptr;
    size_t n = 0;
    int min_cov = 0;
    unsigned lq_max_len = 0;
    bool done = false;
    std::vector<uint32_t> words, wins;   // pos << 8 | char; (start, end) pairs
    uint32_t counts[5] = {0, 0, 0, 0, 0};  // len, uncorrected_len, lstrip, rstrip, lqseq_total_length
};

// Thrown when a device (or pinned host) allocation fails for lack of memory.  The C ABI catches it, releases the
// context's buffers, retries with half the piles and -- for a single pile that still does not fit -- reports the
// reference's out-of-memory seed (len == 3, lib/nextcorrect.c:2254-2261).  Every other HIP error aborts with a message.
struct DeviceOom {
    size_t bytes;
};

class DeviceAligner {
  public:
    static constexpr int kMaxContexts = 16;
    static DeviceAligner &instance();          // context 0
    static DeviceAligner &context(int i);
    static DeviceAligner *peek(int i);  // nullptr if context i was never used
    static RuntimeStats total_stats();
    // device memory plan of one batch call over `drivers` contexts: sets their trace budgets, returns the column budget of a sub-batch
    static void plan_memory(int drivers, uint64_t *tag_budget);
    static void level_buffers(int drivers);             // after a batch call: every context up to the largest sizes any context met
    static void reserve_device_memory(uint64_t bytes);  // left free by every later plan (another stage's working set)
    static void reset_all_stats();
    void align_batch(AlnJob **jobs, size_t n);
    // the same alignments, but what comes back is each job's summary and its runs (K15) instead of a byte per column: res[i] for
    // jobs[i], runs = every job's CIGAR back to back (res[i].run_off); the jobs' own result fields stay untouched
    void align_batch_runs(AlnJob **jobs, size_t n, AlnRunsResult *res, std::vector<uint32_t> &runs);
    // device main phase / candidate extraction of a batch of piles (see Backend in nd_host.h);
    // begin_batch()/end_batch() bracket one batch and serialise batches of one process
    // order: who goes first when several callers wait for this context (lower first; equal: any) -- the calls of a process take a
    // number each (next_order), so that a context serves the older of two batch calls in flight before the newer one
    void begin_batch(uint64_t order = 0, bool reserved = false);
    // a thread that will bring this context several batches of one call keeps its place in the line between them
    void reserve_batches(uint64_t order);
    void unreserve_batches(uint64_t order);
    static uint64_t next_order();
    void run_main(MainPile **piles, size_t n);
    // offer_rank: piles that ask for it (ExtractPile::rank) get their regions ranked by K14 behind K11
    void run_extract(ExtractPile **piles, size_t n, bool offer_rank = true);
    void run_rank(RankReq *reqs, size_t n);   // the batched entry's problems: one pool up, one copy back
    void run_cns(CnsReq *reqs, size_t n);     // the batched entry's walks through K20; req.done = false: declined, the host routine takes it
    void run_cns_walk(CnsWalkReq *reqs, size_t n);   // ... of modes 1 and 2 through K21
    void run_phase(PhaseReq *reqs, size_t n);        // the batched entry's HiFi piles through K22: one pool up, the records back
    void run_splice(SpliceReq **reqs, size_t n);     // the splices of the batched entry or of the engine through K24: four arenas up, records and strings back
    void run_lq(LqRound **rounds, size_t n);
    // req.done = false: declined, the caller's host path takes it.  form 0: NDGPU_POA_RESIDENT decides; 1: resident graphs (K19);
    // 2: K13's rounds with the graphs on the host
    void run_poa(PoaReq **reqs, size_t n, int form = 0);
    void end_batch();
    // resident read DB: every ndgpu_db handle owns its device copy (upload_db / free_db); a batch names the one its
    // AlnJob::q_dev / t_dev and MainPile::dev_off index into (use_db; nullptr: sequences come with the batch)
    static uint32_t *upload_db(const uint32_t *pool_words, size_t n_words, int device);  // nullptr: out of device memory
    static void free_db(uint32_t *dev_pool);
    void use_db(const uint32_t *dev_pool);
    int device() const;
    void set_host_threads(int n);   // threads used for packing / decoding inside a batch
    // after a DeviceOom: wait for the stream, drop every grow-only buffer of this context (they are re-created on demand)
    void release_memory();
    // after a DeviceOom: drop the process-wide "largest size any context held of a buffer" marks, so that the retry of a smaller
    // range asks for what IT needs and not for what just failed
    static void forget_sizes();
    // the public entry's form: only when no batch is open on this context (a batch keeps its main-phase buffers alive from
    // run_main to end_batch, between the calls that hold the context's lock); false = the context is busy, nothing released
    bool release_memory_if_idle();
    void *stream() const;
    RuntimeStats stats() const;
    void reset_stats();

  private:
    DeviceAligner();
    ~DeviceAligner();
    void run_chunk(AlnJob **jobs, size_t n);
    void run_chunk_runs(AlnJob **jobs, size_t n, AlnRunsResult *res, std::vector<uint32_t> &runs);
    // what both have in common: tasks built and uploaded, K7 / K8a launched, the AlnOut records (and the ops, if asked) on the host,
    // the wide-band tasks run again; returns the chunk's ops words
    uint64_t chunk_front(AlnJob **jobs, size_t n, std::vector<uint8_t> &bad, bool ops_to_host, uint64_t *dev_ns);
    struct State;
    State *s_;
};

// The product's only Backend: every request runs in HIP kernels on the device.
class HipBackend : public Backend {
  public:
    explicit HipBackend(int ctx = 0, int host_threads = 1, const uint32_t *db_pool = nullptr, uint64_t order = ~0ull, bool reserved = false)
        : dev_(DeviceAligner::context(ctx)) {
        dev_.begin_batch(order == ~0ull ? DeviceAligner::next_order() : order, reserved);
        dev_.set_host_threads(host_threads);
        dev_.use_db(db_pool);
    }
    ~HipBackend() override { finish(); }
    void run_main(MainPile **piles, size_t n) override { dev_.run_main(piles, n); }
    void run_extract(ExtractPile **piles, size_t n) override {
        static const bool host_rank = getenv("NDGPU_RANK_HOST") != nullptr;  // test hook: no ranking offered, the engine ranks on the host
        dev_.run_extract(piles, n, !host_rank);
    }
    void run_rank(RankReq *reqs, size_t n) { dev_.run_rank(reqs, n); }
    void run_cns(CnsReq *reqs, size_t n) { dev_.run_cns(reqs, n); }
    void run_cns_walk(CnsWalkReq *reqs, size_t n) { dev_.run_cns_walk(reqs, n); }
    void run_phase(PhaseReq *reqs, size_t n) { dev_.run_phase(reqs, n); }
    bool run_splice(SpliceReq **reqs, size_t n) override {
        static const bool host_splice = getenv("NDGPU_SPLICE_HOST") != nullptr;  // test hook: a backend without the entry
        if (host_splice) return false;
        dev_.run_splice(reqs, n);
        return true;
    }
    void run_align(AlnJob **jobs, size_t n) override { dev_.align_batch(jobs, n); }
    void run_align_runs(AlnJob **jobs, size_t n, AlnRunsResult *res, std::vector<uint32_t> &runs) { dev_.align_batch_runs(jobs, n, res, runs); }
    bool run_lq(LqRound **rounds, size_t n) override {
        static const bool host_lq = getenv("NDGPU_LQ_HOST") != nullptr;  // test hook: the host path of the rounds
        if (host_lq) return false;
        dev_.run_lq(rounds, n);
        return true;
    }
    bool run_poa(PoaReq **reqs, size_t n) override {
        static const bool host_poa = getenv("NDGPU_POA_HOST") != nullptr;  // test hook: every POA problem on the host
        if (host_poa) return false;
        dev_.run_poa(reqs, n);
        return true;
    }
    void run_poa_form(PoaReq **reqs, size_t n, int form) { dev_.run_poa(reqs, n, form); }   // the flags entry's choice of form
    void end_batch() override { finish(); }

  private:
    void finish() {
        if (open_) dev_.end_batch();
        open_ = false;
    }
    DeviceAligner &dev_;
    bool open_ = true;
};

}  // namespace ndgpu
