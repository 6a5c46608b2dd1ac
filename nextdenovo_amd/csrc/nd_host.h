// Host-side declarations of the MI355X read-correction engine (internal; the
// public C ABI is include/ndgpu_nextcorrect.h).
#pragma once

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <string>
#include <thread>
#include <vector>

#include "nd_phase.h"
#include "nd_splice.h"

namespace ndgpu {

// ABI-compatible with the reference's `consensus_trimed` (lib/nextcorrect.h:70-74).
struct ConsensusTrimed {
    unsigned int len;
    float identity;
    char *seq;
};

// Column kinds of a pairwise alignment, as produced by the HIP traceback kernel.
enum : uint8_t { OP_MATCH = 0, OP_QONLY = 1, OP_TONLY = 2 };

enum : int { ALN_NONE = 0, ALN_OK = 1, ALN_GAP_ABORT = 2 };

// One query-vs-target alignment request.  Sequences are ASCII on the host side;
// the device runtime packs them to 2 bit.  `hq` selects the align_hq
// thresholds (lib/align.c:563-570) instead of align (:572-578).
struct AlnJob {
    const char *q = nullptr;
    int q_len = 0;
    const char *t = nullptr;
    int t_len = 0;
    int hq = 0;
    // optional: `t` points into a larger buffer shared by many jobs (the seed); the
    // runtime then packs/uploads that buffer once
    const char *t_owner = nullptr;
    int t_owner_len = 0;
    // optional: base offsets of q[0] / t[0] inside the device-resident read DB
    // (ReadDb); when >= 0 nothing is packed or uploaded for that sequence
    int64_t q_dev = -1;
    int64_t t_dev = -1;
    // optional: q already packed (2 bit per base, 16 bases per word, first base in the low bits: pack_2bit_lsb below)
    const uint32_t *q_words = nullptr;
    // results
    int status = ALN_NONE;
    int q_used = 0;            // aln_q_len
    int t_used = 0;            // aln_t_len
    std::vector<uint8_t> ops;  // forward column kinds (empty unless ALN_OK)
};

// What the batched alignment entry reports per job (DeviceAligner::align_batch_runs): align()'s outcome, the counts of its columns
// and its CIGAR as job.n_runs words from runs[job.run_off] on -- length << 4 | op in BAM numbering, 7 '=' / 1 'I' / 2 'D'.
struct AlnRunsResult {
    int status = ALN_NONE;
    uint32_t aln_len = 0, q_used = 0, t_used = 0;
    uint32_t n_match = 0, n_ins = 0, n_del = 0, max_gap_run = 0;
    uint32_t n_runs = 0;
    uint64_t run_off = 0;
};
// The same summary from one byte per column -- the host form of K15 (ond_kernels.hip), what the batched entry's host flag reports:
// runs of equal kinds, appended to `runs`; status, q_used and t_used are the caller's.  (Inline: a stand-alone sanitizer program of
// the tests includes this header and nothing else.)
inline void aln_runs_host(const uint8_t *ops, size_t n_cols, AlnRunsResult &r, std::vector<uint32_t> &runs) {
    r.aln_len = (uint32_t)n_cols;
    r.n_match = r.n_ins = r.n_del = r.max_gap_run = r.n_runs = 0;
    r.run_off = runs.size();
    for (size_t a = 0; a < n_cols;) {
        size_t b = a + 1;
        while (b < n_cols && ops[b] == ops[a]) b++;
        const uint32_t len = (uint32_t)(b - a);
        if (ops[a] == OP_MATCH) r.n_match += len;
        else {
            (ops[a] == OP_QONLY ? r.n_ins : r.n_del) += len;
            if (len > r.max_gap_run) r.max_gap_run = len;
        }
        runs.push_back(len << 4 | (ops[a] == OP_MATCH ? 7u : ops[a] == OP_QONLY ? 1u : 2u));
        r.n_runs++;
        a = b;
    }
}

// One visited cell of the main MSA's best_pp walk, origin first (device: PathItem).
struct PathStep {
    int32_t t_pos;
    uint16_t delta;
    uint8_t base;   // A0 T1 G2 C3 -4 N5 (lib/nextcorrect.c:52-62)
    uint16_t link;  // best_link_count of the cell
    uint16_t cov;   // coverage of the column
};

// Main-phase request of one pile: align every read to its seed window, build the MSA
// link graph, score it and walk best_pp (lib/nextcorrect.c:2271-2293, 2130-2202).
// Executed entirely on the device by the HIP backend.
struct MainPile {
    // inputs
    unsigned n = 0;                      // records, [0] = the seed
    const char *const *seqs = nullptr;   // ASCII sequences, or nullptr when dev_off is used
    const unsigned *seq_len = nullptr;
    const unsigned *aln_start = nullptr;
    const unsigned *aln_end = nullptr;
    const int64_t *dev_off = nullptr;    // ReadDb pool offsets of seqs[i][0], or nullptr
    unsigned min_len_aln = 500, max_cov_aln = 130;
    int factor = 3;
    int hq = 0;
    // optional: the engine would take the walk's consensus words and low-quality windows (cns_windows_host of nd_cns.h) instead of
    // the walk itself
    bool want_cns = false;
    int cns_mode = 0;                    // which loop, where want_cns: 0 raw reads (cns_windows_host), 1 HiFi (cns_kmer_host), 2 -fast (cns_fast_host)
    int min_cov = 0;
    unsigned lq_max_len = 0;
    // outputs
    std::vector<PathStep> path;
    unsigned n_aligned = 0;              // reads that entered the MSA (incl. the seed)
    int slot = -1;                       // backend-private handle, valid until end_batch()
    // optional output, where want_cns and the backend offers it: cns_words[p] = pos << 8 | char of the p-th non-gap step, cns_windows =
    // (start, end) pairs in emission order, cns_counts = len, uncorrected_len, lstrip, rstrip, lqseq_total_length; `path` stays empty.
    // A backend that does not fill these leaves cns_ready false, and the engine takes the walk.
    bool cns_ready = false;
    std::vector<uint32_t> cns_words, cns_windows;
    uint32_t cns_counts[5] = {0, 0, 0, 0, 0};
    // cns_mode 2: cns_fast = lq_m, hq_m, lq_total_len, characters emitted; cns_seq = the stretch [lq_m, hq_m), reversed
    uint32_t cns_fast[4] = {0, 0, 0, 0};
    std::string cns_seq;
};

// Candidate strings of one low-quality region (lib/nextcorrect.c:373-404).
struct RegionReq {
    unsigned start = 0, end = 0;         // inclusive seed columns
    unsigned max_len = 0;                // lqseq_max_length
    unsigned max_len0 = 0;               // limit for the seed's own candidate (0: same as max_len)
    std::vector<std::string> cands;      // <= 40, in pile order
    std::vector<uint16_t> cand_rank;     // source read of each candidate (index among aligned reads)
    unsigned n_large = 0;                // reads longer than max_len - 1 seen before the 40th candidate
    // optional: the 8-mer ranking of `cands` (lq_rank_host below), where ExtractPile::rank asked for it and the backend offers it.
    // A backend that does not fill these leaves ranked false, and the engine ranks on the host.
    bool ranked = false;
    uint8_t rank_tail = 0;               // the tail windows were ranked too
    uint8_t rank_order[40] = {0};        // candidate index at rank r
    uint16_t rank_kscore[40] = {0};      // its score
    // optional: the HiFi phasing and ranking of `cands` (hifi_phase_host of nd_phase.h), where ExtractPile::phase asked for it and the
    // backend offers it.  A backend that does not fill the record leaves phased false, and the engine runs the rule on the host.
    bool phased = false;
    PhaseRecord phase;
};

struct ExtractPile {
    int slot = -1;
    bool rank = false;                   // the engine would take a ranking of every region with five or more candidates
    bool phase = false;                  // (HiFi) the engine would take the phasing records of the pile's regions
    unsigned n_aligned = 0;              // ... of a pile with this many aligned reads (MainPile::n_aligned)
    std::vector<RegionReq> regions;
};

// The 8-mer ranking of a low-quality region's candidates (lib/nextcorrect.c:281-337, 405-440): n sequences (1..40) in input order ->
// order[r] = input index of the sequence at rank r, kscore[r] = its score, tail = whether the tail windows were ranked too.
constexpr int kLqRankMax = 40;           // LQ_CAN_MAX
void lq_rank_host(const char *const *seqs, const uint16_t *len, int n, uint8_t *order, uint16_t *kscore, int *tail);

// One ranking problem of the batched entry (DeviceAligner::run_rank)
struct RankReq {
    const char *const *seqs = nullptr;
    const uint16_t *len = nullptr;
    int n = 0;
    uint8_t order[40] = {0};
    uint16_t kscore[40] = {0};
    int tail = 0;
};

// One low-quality-region round of a pile (generate_consensus_trimed + get_lqseqs_from_align_tags, lib/nextcorrect.c:1538-1669,
// 1250-1338) as a device request: align the jobs, link the regions' pseudo-seeds with 'N' columns, second MSA over the
// <= 30 rows, scoring DP, walk.  A backend that cannot serve it (or declines a pile: ok = false) leaves the round to the host
// path (run_align on the same jobs + the engine's own MSA).
struct LqRound {
    struct Piece {
        int job;                          // index into *jobs, -1: nothing to align in this (row, region) slot
        unsigned sl;                      // pseudo-seed length of the region
    };
    std::vector<AlnJob> *jobs = nullptr;  // q / q_len / q_words, t / t_len (the region's pseudo-seed), hq
    std::vector<Piece> pieces;            // row-major: 30 rows x n_regions, regions in the reference's (descending) order
    unsigned n_regions = 0;
    int factor = 2, qv_factor = 5;        // lib/nextcorrect.c:1262, 1303
    // outputs
    bool ok = false;
    std::string lqc;                      // the walk's characters, origin first
};

// ASCII [ACGT]* -> 2 bit per base, 16 bases per word, first base in the low bits (the device's sequence pools); false on any
// other byte.  out must hold (n + 15) / 16 words.
bool pack_2bit_lsb(uint32_t *out, const char *s, size_t n);

struct PoaReq;   // one POA problem as a backend request (below)

// The end of a pile as a backend request (Backend::run_splice; the jobs of ndgpu_splice_batch take the same form): the integers
// splice_host and ssr_trim_host (nd_splice.h) give for it, and the result string.
struct SpliceReq {
    const uint32_t *words = nullptr;       // pos << 8 | char, ascending positions; [lstrip, len - rstrip) is read
    uint32_t len = 0, lstrip = 0, rstrip = 0;
    const SpliceRegion *regions = nullptr;
    size_t n_regions = 0;
    bool hifi = false;
    bool done = false;                     // false: declined, the host statement takes the job
    uint32_t out_len = 0, lq_m = 0, hq_m = 0, lq_total_len = 0;
    int32_t lq_i = 0, clip_s = 0, clip_e = 0;
    uint32_t code = 0, trimmed = 0;        // code: 0, 2 (HiFi, all lower case) or 4 (the clips leave 10 bases or fewer)
    std::string seq;
};

// Executes the device-side work of a batch of piles.  The product has exactly one
// implementation (HipBackend, device_runtime.hip); tests plug the CPU oracle here to
// exercise the host logic without a GPU.
class Backend {
  public:
    virtual ~Backend() {}
    virtual void run_main(MainPile **piles, size_t n) = 0;
    virtual void run_extract(ExtractPile **piles, size_t n) = 0;
    virtual void run_align(AlnJob **jobs, size_t n) = 0;
    // low-quality-region rounds on the backend; false: not offered (every round goes the host way)
    virtual bool run_lq(LqRound **rounds, size_t n) { (void)rounds; (void)n; return false; }
    // a batch of POA problems on the backend; false: not offered (the caller computes every one on the host)
    virtual bool run_poa(PoaReq **reqs, size_t n) { (void)reqs; (void)n; return false; }
    // the piles' final splices on the backend; false: not offered.  A request whose done stays false is the caller's to compute.
    virtual bool run_splice(SpliceReq **reqs, size_t n) { (void)reqs; (void)n; return false; }
    virtual void end_batch() = 0;  // releases whatever run_main kept for run_extract
};

struct CorrectParams {
    unsigned max_mem_len = 0;
    unsigned min_len_aln = 500;
    unsigned max_cov_aln = 130;
    unsigned min_cov = 4;
    unsigned lqseq_max_length = 10000;
    float min_error_corrected_ratio = 0.8f;
    unsigned split = 0;
    unsigned fast = 0;
    int read_type = 1;  // 1 ont, 2 clr, 3 hifi
};

std::string poa_consensus(const std::vector<std::string> &seqs);

// The same consensus taken one sequence at a time (poa.cpp), so that a batch of problems can hand the one O(X * Y) step -- the
// alignment of a sequence against the graph, up to and including its route -- to the device in lockstep rounds
// (DeviceAligner::run_poa) while graph growth, topological order and heaviest path stay on the host.  poa_consensus() is
// start() + add_sequence() for every further sequence + consensus().
struct PoaRows {                      // the graph as an alignment sees it: row i + 1 = the i-th node in topological order
    std::vector<uint8_t> base, sink;  // the node's byte (compared as a byte: the NUL-tail node matches nothing); it has no out-edge
    std::vector<uint32_t> pred_off;   // rows() + 1 offsets into preds
    std::vector<uint16_t> preds;      // predecessor rows in in-edge insertion order (row 0 for a node without in-edges)
};
class PoaGraph {
  public:
    PoaGraph();
    ~PoaGraph();
    PoaGraph(const PoaGraph &) = delete;
    PoaGraph &operator=(const PoaGraph &) = delete;
    void start(const char *s, size_t len);                  // the first sequence: a chain
    size_t rows() const;                                     // X: nodes of the graph
    void export_rows(PoaRows &out);                          // "export rows"
    void set_route(const uint32_t *walk, size_t n);          // "align", done elsewhere: the route in walk order (see poa.cpp)
    bool thread(int seq, const char *s, int len);            // "thread + toposort"; false: the graph outgrew its 16-bit node ids
    void add_sequence(int seq, const char *s, int len);      // all three on the host
    std::string consensus(int nseq);                         // heaviest path, cut at the first NUL

  private:
    struct Impl;
    Impl *impl_;
};

// One POA problem as a backend request (Backend::run_poa).  done: `out` holds what poa_consensus(seqs) returns; otherwise the
// backend declined the problem (outside the device's limits or its memory plan) and the caller computes it on the host.
struct PoaReq {
    std::vector<std::string> seqs;
    std::string out;
    bool done = false;
    bool failed = false;   // no path can compute it: more than 64 sequences, or a graph beyond 65,535 nodes
};
constexpr int kPoaMaxSeqs = 64;       // labels are one bit per sequence in a 64-bit word
constexpr int kPoaMaxSeqLen = 9999;   // the reference's struct seq_ (lib/nextcorrect.h:63-68)

class PileImpl;

// Per-seed consensus state machine.  Device work is exposed as requests so that many
// piles share each launch:
//     MAIN (MainPile) -> EXTRACT (ExtractPile) [-> POA (PoaReq)] -> LQ round 1 (AlnJob) -> LQ round 2 [-> SPLICE (SpliceReq)] -> DONE
class PileEngine {
  public:
    // POA: between EXTRACT and LQ round 1, when the regions' POA problems go out as requests; SPLICE: behind the last LQ round, when
    // the splice goes out as a request (NDGPU_SPLICE_DEVICE=1)
    enum Phase { MAIN = 0, EXTRACT = 1, LQ_ROUND = 2, DONE = 3, POA = 4, SPLICE = 5 };
    // ASCII form (the nextCorrect ABI): seqs[i] NUL-terminated.
    PileEngine(const char *const *seqs, const unsigned *aln_start, const unsigned *aln_end, unsigned seq_count,
               const CorrectParams &prm);
    // Resident-DB form: only lengths and ReadDb pool offsets, no host copy of the reads
    // (`seed` = ASCII copy of the seed itself, needed by the HiFi consensus only; may be null).
    PileEngine(const unsigned *seq_len, const int64_t *dev_off, const unsigned *aln_start, const unsigned *aln_end,
               unsigned seq_count, const CorrectParams &prm, const char *seed = nullptr);
    ~PileEngine();
    PileEngine(const PileEngine &) = delete;
    PileEngine &operator=(const PileEngine &) = delete;

    Phase phase() const;
    bool done() const { return phase() == DONE; }
    MainPile *main_request();        // valid in MAIN
    ExtractPile *extract_request();  // valid in EXTRACT
    void collect_jobs(std::vector<AlnJob *> &out);  // LQ_ROUND (host path)
    LqRound *lq_request();           // LQ_ROUND: the round as one device request (nullptr: nothing to hand over)
    void collect_poa(std::vector<PoaReq *> &out);   // POA: the regions' problems
    SpliceReq *splice_request();     // valid in SPLICE
    void advance();                  // consume the finished request(s), move on
    ConsensusTrimed *take_result();  // malloc'd, caller frees with free_consensus_trimed

  private:
    PileImpl *impl_;
};

// Wall-clock accounting of the host driver (summed over driver threads), NDGPU_PROF=1 prints it.
struct HostProf {
    std::atomic<uint64_t> main_ns{0}, extract_ns{0}, align_ns{0}, advance_ns{0}, build_ns{0}, jobs{0};
    std::atomic<uint64_t> m_prep{0}, m_aln{0}, m_tags{0}, m_msa{0}, m_post{0};  // inside run_main
    std::atomic<uint64_t> adv_ns[4] = {{0}, {0}, {0}, {0}};  // CPU time inside PileEngine::advance by phase (summed over threads)
    std::atomic<uint64_t> rank_ns{0}, poa_ns{0}, lqstart_ns{0};  // inside "after extract": 8-mer ranking, POA, laying out LQ round 1
    std::atomic<uint64_t> c_pack{0}, c_dev{0}, c_decode{0}, c_jobs{0};  // LQ-stage alignment batches: host packing / device round trip / host decoding
};
extern HostProf g_prof;

// The CPUs this process can actually have: the smaller of the hardware threads, the scheduling affinity and the cgroup CPU quota
// (cpu.max / cpu.cfs_quota_us).  A container on a 256-thread host with a quota of 16 CPUs that starts 256 busy threads spends its
// quota in the first quarter of every 100 ms period and is then throttled as a whole -- the threads that launch kernels included.
int effective_cpus();

// Host cores are shared by the driver threads of all device contexts: each host section is guaranteed its base share and
// borrows the cores that no other section is using at that moment (the tail of a call, when few contexts are still
// busy, would otherwise run on an eighth of the machine).  total = 0 switches borrowing off.
struct CoreGovernor {
    static void set_total(int total);
    static int acquire(int base);    // threads granted (>= base)
    static void release(int granted);
};
struct CoreLease {
    int n;
    explicit CoreLease(int base) : n(CoreGovernor::acquire(base)) {}
    ~CoreLease() { CoreGovernor::release(n); }
    CoreLease(const CoreLease &) = delete;
    CoreLease &operator=(const CoreLease &) = delete;
};

// The two host pools, both on a CoreLease of `base` threads held for the loop.  small: not worth a thread -- the caller's thread
// does everything and no lease is taken; max_threads: what the amount of work justifies; every call site passes its own thresholds.
// f(begin, end) over contiguous ranges of [0, n): one range a thread, the caller's thread waits.
template <typename F>
void host_ranges(size_t n, bool small, int base, size_t max_threads, F f) {
    if (small) {
        f((size_t)0, n);
        return;
    }
    CoreLease lease(base);
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)lease.n, max_threads));
    std::vector<std::thread> th;
    for (size_t t = 0; t < nt; t++) th.emplace_back(f, n * t / nt, n * (t + 1) / nt);
    for (auto &x : th) x.join();
}
// f(i) for every i of [0, n): a thread claims the next index when it is done with the last.  caller_works: the caller's thread is
// one of the threads, else it waits.
template <typename F>
void host_each(size_t n, bool small, int base, size_t max_threads, bool caller_works, F f) {
    if (small) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    CoreLease lease(base);
    const size_t nt = std::max<size_t>(1, std::min<size_t>((size_t)lease.n, max_threads));
    std::atomic<size_t> next(0);
    auto work = [&] {
        for (size_t i; (i = next.fetch_add(1)) < n;) f(i);
    };
    std::vector<std::thread> th;
    for (size_t t = caller_works ? 1 : 0; t < nt; t++) th.emplace_back(work);
    if (caller_works) work();
    for (auto &x : th) x.join();
}

// Drives a set of engines to completion over one backend (host phases on `threads`).
void run_engines(PileEngine **eng, size_t n, Backend &be, int threads);

ConsensusTrimed *make_error_seed(unsigned len);

// Read database kept resident in HBM for the lifetime of a correction run: every
// read forward AND reverse-complemented, 2 bit per base, LSB-first words (the device
// packing of nd_device.h), so that any strand-corrected overlap substring
// (reference: getseq/subbit_, lib/ovlseq.c:39-48, lib/bseq.c:241-255) is a plain
// window of the pool -- no per-pile extraction or upload.
class ReadDb {
  public:
    // `words`: reference .2bit payload layout (lib/bseq.c:114-139): 16 bases per
    // uint32, first base in the two most significant bits; read i starts at
    // words[word_off[i]] and has len[i] bases.
    ReadDb(uint32_t n_reads, const uint32_t *words, const uint64_t *word_off, const uint32_t *len);
    uint32_t n_reads() const { return (uint32_t)len_.size(); }
    uint32_t length(uint32_t r) const { return len_[r]; }
    // pool offset (bases) of base `start` of the window [start, end] of read r, after
    // optional reverse-complement of the window
    int64_t window_offset(uint32_t r, uint32_t start, uint32_t end, int rev) const {
        return rev ? (int64_t)(rc_off_[r] + (len_[r] - 1 - end)) : (int64_t)(fwd_off_[r] + start);
    }
    // ASCII copy of the same window (host side)
    std::string window(uint32_t r, uint32_t start, uint32_t end, int rev) const;
    const std::vector<uint32_t> &pool() const { return pool_; }
    uint64_t total_bases() const { return total_; }

  private:
    std::vector<uint32_t> pool_;
    std::vector<uint64_t> fwd_off_, rc_off_;
    std::vector<uint32_t> len_;
    uint64_t total_ = 0;
};

}  // namespace ndgpu
