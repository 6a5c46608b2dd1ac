// Per-seed consensus engine (host side).
//
// Everything the reference does inside nextCorrect() (lib/nextcorrect.c:2219-2305)
// EXCEPT the pairwise O(ND) alignments, which are requested as AlnJob batches and
// executed by the HIP kernels (csrc/ond_kernels.hip).  The logic here reproduces
// the reference's observable behaviour bit for bit (tie-breaks, integer/float
// conversions, first-seen ordering) but on our own data layout:
//   * alignments arrive as column-kind streams (match / query-only / target-only)
//     instead of two gapped strings,
//   * the MSA link graph is one flat cell table + one link arena per pile
//     (index-linked lists) instead of per-column malloc blocks,
//   * low-quality regions keep std::string sequences instead of 10 kB slots,
//   * sorting uses std::stable_sort, which yields the same permutation as glibc's
//     merge-sort qsort() on the reference's comparators.
// Reference locations are cited at each step.
#include "nd_host.h"
#include "nd_cns.h"
#include "nd_splice.h"

#include <algorithm>
#include <cctype>
#include <climits>
#include <cstdio>
#include <cstdlib>
#include <atomic>
#include <chrono>
#include <cstring>
#include <thread>
#include <cmath>
#include <sched.h>

namespace ndgpu {
static inline uint64_t now_ns();

ConsensusTrimed *make_error_seed(unsigned len) {
    // lib/nextcorrect.c:261-266.  The reference leaves the buffer uninitialised;
    // callers only look at `len` (lib/nextcorrect.py:236,255).  We zero it.
    ConsensusTrimed *c = (ConsensusTrimed *)malloc(sizeof(ConsensusTrimed));
    c->len = len;
    c->identity = 0;
    c->seq = (char *)calloc(len + 1, 1);
    return c;
}

namespace {

// lib/nextcorrect.c:42-62
const unsigned char kIntToBase[7] = {'A', 'T', 'G', 'C', '-', 'N', 'M'};
struct BaseLut {
    uint8_t v[256];
    BaseLut() {
        memset(v, 4, sizeof(v));
        v['A'] = v['a'] = 0;
        v['T'] = v['t'] = 1;
        v['G'] = v['g'] = 2;
        v['C'] = v['c'] = 3;
        v['N'] = 5;
        v['M'] = 6;
    }
};
const BaseLut kLut;
inline uint8_t base_code(char c) { return kLut.v[(unsigned char)c]; }

struct Tag {
    int32_t t_pos;
    uint16_t delta;
    uint8_t base;
};

struct TagList {
    unsigned aln_t_s = 0;
    std::vector<Tag> tags;
};

struct Link {
    int32_t pp_t;
    int32_t ppp_t;
    uint16_t pp_d;
    uint16_t ppp_d;
    uint8_t pp_b;
    uint8_t ppp_b;
    uint16_t count;
    int32_t next;
    int64_t score;
};

struct Cell {
    int32_t head = -1, tail = -1;
    uint32_t len = 0;
    int64_t best_score = 0;
    int32_t best_t = 0;  // calloc-zero initial state (lib/nextcorrect.c:181)
    uint16_t best_d = 0;
    uint8_t best_b = 0;
    uint16_t best_link = 0;
};

struct Pos {
    int32_t t;
    uint16_t d;
    uint8_t b;
};

// Flat MSA link graph of one (pseudo-)seed.
struct Msa {
    std::vector<uint16_t> max_size, coverage;
    std::vector<uint32_t> cell_base;
    std::vector<Cell> cells;
    std::vector<Link> links;

    explicit Msa(size_t ncol) : max_size(ncol, 0), coverage(ncol, 0) {}
    size_t ncol() const { return max_size.size(); }
    Cell &cell(int32_t t, unsigned d, unsigned b) { return cells[cell_base[t] + d * 6 + b]; }

    // lib/nextcorrect.c:175-198
    void allocate() {
        cell_base.resize(ncol() + 1);
        uint32_t acc = 0;
        for (size_t p = 0; p < ncol(); p++) {
            cell_base[p] = acc;
            acc += (uint32_t)max_size[p] * 6;
        }
        cell_base[ncol()] = acc;
        cells.assign(acc, Cell());
    }

    // lib/nextcorrect.c:212-250: count (pp,ppp) predecessor pairs per cell,
    // keeping first-seen order inside each cell.
    void count_links(const std::vector<TagList> &reads) {
        size_t total = 0;
        for (const TagList &r : reads) total += r.tags.size();
        links.reserve(total / 4 + 16);
        const Tag head{-1, 0, 0};
        for (const TagList &r : reads) {
            const size_t n = r.tags.size();
            for (size_t i = 0; i < n; i++) {
                const Tag &cur = r.tags[i];
                const Tag &pp = i > 0 ? r.tags[i - 1] : head;
                const Tag &ppp = i > 1 ? r.tags[i - 2] : head;
                if (cur.base == 6 || pp.base == 6) continue;
                Cell &c = cell(cur.t_pos, cur.delta, cur.base);
                int32_t at = c.head;
                while (at != -1) {
                    Link &l = links[at];
                    if (l.pp_t == pp.t_pos && l.pp_d == pp.delta && l.pp_b == pp.base && l.ppp_t == ppp.t_pos &&
                        l.ppp_d == ppp.delta && l.ppp_b == ppp.base) {
                        l.count++;
                        break;
                    }
                    at = l.next;
                }
                if (at == -1) {
                    Link l;
                    l.pp_t = pp.t_pos; l.pp_d = pp.delta; l.pp_b = pp.base;
                    l.ppp_t = ppp.t_pos; l.ppp_d = ppp.delta; l.ppp_b = ppp.base;
                    l.count = 1; l.score = 0; l.next = -1;
                    int32_t id = (int32_t)links.size();
                    links.push_back(l);
                    if (c.tail == -1) c.head = id;
                    else links[c.tail].next = id;
                    c.tail = id;
                    c.len++;
                }
            }
        }
    }

    // lib/nextcorrect.c:1263-1300 (second, low-quality-region MSA): 6 symbols,
    // plain max, origin = last cell.
    Pos score_lq(int factor) {
        Pos origin{-1, 0, 0};
        const int ncols = (int)ncol();
        for (int p = 0; p < ncols; p++) {
            const int64_t penalty = (int64_t)factor * coverage[p];
            for (unsigned d = 0; d < max_size[p]; d++) {
                for (unsigned b = 0; b < 6; b++) {
                    Cell &c = cell(p, d, b);
                    c.best_score = -10;
                    c.best_t = -1;
                    for (int32_t m = c.head; m != -1; m = links[m].next) {
                        Link &lm = links[m];
                        if (lm.pp_t == -1) {
                            lm.score = 10 * (int64_t)lm.count - penalty;
                        } else {
                            const Cell &pc = cell(lm.pp_t, lm.pp_d, lm.pp_b);
                            for (int32_t n = pc.head; n != -1; n = links[n].next) {
                                const Link &ln = links[n];
                                if (ln.pp_t != lm.ppp_t || ln.pp_d != lm.ppp_d || ln.pp_b != lm.ppp_b) continue;
                                int64_t s = ln.score + 10 * (int64_t)lm.count - penalty;
                                if (s > lm.score) lm.score = s;
                            }
                        }
                        if (lm.score > c.best_score || (lm.score == c.best_score && lm.pp_b != 4)) {
                            c.best_score = lm.score;
                            c.best_t = lm.pp_t; c.best_d = lm.pp_d; c.best_b = lm.pp_b;
                            c.best_link = lm.count;
                        }
                    }
                    origin = Pos{p, (uint16_t)d, (uint8_t)b};
                }
            }
        }
        return origin;
    }
};

// get_align_tags (lib/nextcorrect.c:1485-1536) for an explicit pair of gapped strings.
void tags_from_strings(const std::string &t_str, const std::string &q_str, unsigned aln_t_s, TagList &out, Msa &msa) {
    const size_t n = t_str.size();
    out.aln_t_s = aln_t_s;
    out.tags.resize(n);
    int32_t t = (int32_t)aln_t_s - 1;
    uint16_t delta = 0;
    for (size_t i = 0; i < n; i++) {
        if (t_str[i] != '-') {
            t++;
            delta = 0;
        }
        Tag &g = out.tags[i];
        g.t_pos = t;
        g.delta = delta++;
        g.base = base_code(q_str[i]);
        if (g.delta == 0 && q_str[i] != 'M') msa.coverage[t]++;
        if (g.delta >= msa.max_size[t]) msa.max_size[t] = g.delta + 1;
    }
}

struct LqSeq {
    uint16_t order = 0, kscore = 0, len = 0;
    std::string seq;
    std::vector<uint32_t> packed;  // seq in the device's 2-bit form, made once for both low-quality-region rounds
};

struct LqRegion {
    unsigned start = 0, end = 0;
    int len = 0;
    uint8_t indexs = 0, indexe = 0;
    unsigned lqcount = 0;
    unsigned sudoseed_len = 0;
    bool has_seed = false;
    std::string sudoseed;  // sudoseed_len valid bytes
    std::vector<LqSeq> seqs;
};

struct CnsBase {
    unsigned pos;
    char base;
};

struct CnsData {
    unsigned len = 0, uncorrected_len = 0, lstrip = 0, rstrip = 0;
    std::vector<CnsBase> bases;
};

// ---- 8-mer ranking of low-quality-region candidates (lib/nextcorrect.c:281-337)
constexpr int kKmerLen = 8, kKmerRange = 40, kKmerBins = 65536, kKmerMaxSeq = 10;
constexpr int kLqCanMax = 40, kLqSeqMax = 30, kLqRevLen = 2000;

// The 8-mer histogram of the reference lives on the stack and is cleared per call (lib/nextcorrect.c:281-300: 128 KB); a call touches
// at most 40 x 32 of its 65,536 bins, so the clearing -- three to four times per region, tens of thousands of regions per step -- was
// gigabytes of memset.  The bins a call touched are remembered and only those are cleared by the next one.
struct KmerBins {
    std::vector<uint16_t> v = std::vector<uint16_t>(kKmerBins, 0);
    std::vector<uint16_t> touched;
    uint16_t *data() { return v.data(); }
};

// The sequences are seen through seq_bytes / s.len, so that the routines serve the engine's LqSeq records and the plain views of
// lq_rank_host alike.
inline const char *seq_bytes(const LqSeq &s) { return s.seq.data(); }

template <class S>
void count_kmers(const S *seqs, int len, KmerBins &kb, int c, int from_tail) {
    uint16_t *bins = kb.v.data();
    for (uint16_t t : kb.touched) bins[t] = 0;
    kb.touched.clear();
    const int lim = std::min(len, c);
    for (int j = 0; j < lim; j++) {
        const S &s = seqs[j];
        if (s.len < kKmerLen) continue;
        const char *q = seq_bytes(s);
        const int off = from_tail && s.len > kKmerRange ? s.len - kKmerRange : 0;
        const int n = std::min<int>(s.len, kKmerRange) - kKmerLen;
        uint16_t km = 0;
        for (int k = 0; k < n; k++) {
            if (k) km = (uint16_t)(km << 2 | base_code(q[off + k + kKmerLen - 1]));
            else
                for (int x = 0; x < kKmerLen; x++) km = (uint16_t)(km << 2 | base_code(q[off + x]));
            if (bins[km]++ == 0) kb.touched.push_back(km);
        }
    }
}

template <class S>
void count_kscore(S *seqs, int len, const uint16_t *bins, int from_tail) {
    for (int j = 0; j < len; j++) {
        S &s = seqs[j];
        s.kscore = 0;
        if (s.len < kKmerLen) continue;
        const char *q = seq_bytes(s);
        const int off = from_tail && s.len > kKmerRange ? s.len - kKmerRange : 0;
        const int n = std::min<int>(s.len, kKmerRange) - kKmerLen;
        uint16_t km = 0;
        for (int k = 0; k < n; k++) {
            if (k) km = (uint16_t)(km << 2 | base_code(q[off + k + kKmerLen - 1]));
            else
                for (int x = 0; x < kKmerLen; x++) km = (uint16_t)(km << 2 | base_code(q[off + x]));
            s.kscore = (uint16_t)(s.kscore + bins[km]);
        }
    }
}

template <class S>
void sort_by_kscore_desc(S *seqs, int len) {
    // qsort(compare_seq_by_kscore) (lib/nextcorrect.c:254-258,413); glibc qsort is a
    // stable merge sort, so the permutation equals std::stable_sort's.
    std::stable_sort(seqs, seqs + len, [](const S &a, const S &b) { return a.kscore > b.kscore; });
}

void count_kmers(const LqRegion &lq, KmerBins &kb, int c, int from_tail) { count_kmers(lq.seqs.data(), lq.len, kb, c, from_tail); }
void count_kscore(LqRegion &lq, const uint16_t *bins, int from_tail) { count_kscore(lq.seqs.data(), lq.len, bins, from_tail); }
void sort_by_kscore_desc(LqRegion &lq) { sort_by_kscore_desc(lq.seqs.data(), lq.len); }

// The ranking of a raw-read region's candidates, stated once (lib/nextcorrect.c:405-440): the head windows ranked against the first
// candidate, then against the ten best; where the best one is long (or long-ish and scores low) the same over the tail windows
// with candidate 0 in front (find_ref_lqseq: a swap), the two scores added.  K14 (lq_kernels.hip: lq_rank_kernel) computes the same.
struct RankView {
    uint16_t order, kscore, len;
    const char *seq;
};
inline const char *seq_bytes(const RankView &s) { return s.seq; }

void rank_views(RankView *v, int n, KmerBins &bins, int *tail) {
    count_kmers(v, n, bins, 1, 0);
    count_kscore(v, n, bins.data(), 0);
    sort_by_kscore_desc(v, n);
    count_kmers(v, n, bins, kKmerMaxSeq, 0);
    count_kscore(v, n, bins.data(), 0);
    const unsigned kmaxscore = v[0].kscore, kmaxlen = v[0].len;
    *tail = 0;
    if (kmaxlen > 500 || (kmaxlen > 200 && kmaxscore < 200)) {
        *tail = 1;
        uint16_t saved[kLqCanMax];
        if (v[0].order) {
            for (int j = 1; j < n; j++)
                if (!v[j].order) {
                    std::swap(v[0], v[j]);
                    break;
                }
        }
        for (int j = 0; j < n; j++) saved[v[j].order] = v[j].kscore;
        count_kmers(v, n, bins, 1, 1);
        count_kscore(v, n, bins.data(), 1);
        sort_by_kscore_desc(v, n);
        count_kmers(v, n, bins, kKmerMaxSeq, 1);
        count_kscore(v, n, bins.data(), 1);
        for (int j = 0; j < n; j++) v[j].kscore = (uint16_t)(v[j].kscore + saved[v[j].order]);
    }
    sort_by_kscore_desc(v, n);
}

}  // namespace

void lq_rank_host(const char *const *seqs, const uint16_t *len, int n, uint8_t *order, uint16_t *kscore, int *tail) {
    static thread_local KmerBins bins;
    RankView v[kLqCanMax];
    for (int i = 0; i < n; i++) v[i] = RankView{(uint16_t)i, 0, len[i], seqs[i]};
    rank_views(v, n, bins, tail);
    for (int r = 0; r < n; r++) order[r] = (uint8_t)v[r].order, kscore[r] = v[r].kscore;
}

namespace {

struct Result {
    unsigned len = 0;
    float identity = 0;
    std::string seq;
};

}  // namespace

// ---------------------------------------------------------------------------------

class PileImpl {
  public:
    typedef PileEngine::Phase Phase;

    CorrectParams prm;
    unsigned lq_max_len;
    std::vector<std::string> own_seqs;      // ASCII form only
    std::vector<const char *> seq_ptr;
    std::vector<unsigned> seq_len, aln_start, aln_end;
    std::vector<int64_t> dev_off;
    int seed_len = 0;
    Phase phase = PileEngine::MAIN;
    SpliceReq sp_req;                       // the splice as a backend request (NDGPU_SPLICE_DEVICE=1)
    std::vector<uint32_t> sp_words;
    std::vector<SpliceRegion> sp_regions;
    MainPile main;
    ExtractPile extract;
    std::vector<AlnJob> jobs;
    Result result;
    bool error2 = false;
    unsigned n_aligned = 0;

    // state carried through the low-quality-region rounds
    std::vector<LqRegion> regions;
    CnsData cns;
    int lq_iter = 0;          // 1-based round being aligned
    int lq_max_aln_length = 0;
    int lq_max_dif_len = 0;
    struct LqSlot { int i, j, job; };  // (row, region) -> job index or -1 ('M' fill)
    std::vector<LqSlot> lq_slots;
    LqRound lq;               // the round as a device request (HipBackend: K12); lq.ok: its result is in lq.lqc

    std::string seed_copy;  // DB form, HiFi only: the seed's own bases

    PileImpl(const char *const *s, const unsigned *len, const int64_t *dev, const unsigned *st, const unsigned *en,
             unsigned n, const CorrectParams &p, const char *seed_ascii)
        : prm(p) {
        if (seed_ascii) seed_copy = seed_ascii;
        lq_max_len = p.lqseq_max_length > 10000 ? 10000 : p.lqseq_max_length;  // DAG_MAX_LENGTH, nextcorrect.c:2231
        aln_start.assign(st, st + n);
        aln_end.assign(en, en + n);
        if (s) {
            own_seqs.reserve(n);
            for (unsigned i = 0; i < n; i++) own_seqs.emplace_back(s[i]);
            for (unsigned i = 0; i < n; i++) {
                seq_ptr.push_back(own_seqs[i].c_str());
                seq_len.push_back((unsigned)own_seqs[i].size());
            }
        } else {
            seq_len.assign(len, len + n);
            dev_off.assign(dev, dev + n);
        }
        if (n == 0) { finish_error(2); return; }
        seed_len = (int)en[0] + 1;
        // the seed is its own alignment over [aln_start[0], aln_end[0]] (nextcorrect.c:2279-2282);
        // lib/nextcorrect.py always passes 0 .. len-1
        if (st[0] != 0 || seq_len[0] != (unsigned)seed_len) {
            fprintf(stderr, "[ndgpu] seed record must span the whole seed (aln_start 0, aln_end len-1)\n");
            finish_error(2);
            return;
        }
        for (unsigned i = 1; i < n; i++)
            if (en[i] < st[i] || en[i] >= (unsigned)seed_len) {
                fprintf(stderr, "[ndgpu] overlap window outside the seed\n");
                finish_error(2);
                return;
            }
        main.n = n;
        main.seqs = s ? seq_ptr.data() : nullptr;
        main.seq_len = seq_len.data();
        main.aln_start = aln_start.data();
        main.aln_end = aln_end.data();
        main.dev_off = s ? nullptr : dev_off.data();
        main.min_len_aln = prm.min_len_aln;
        main.max_cov_aln = prm.max_cov_aln;
        main.factor = prm.read_type == 3 ? 4 : 3;  // nextcorrect.c:2147
        main.hq = prm.read_type == 3;              // align_hq for HiFi, nextcorrect.c:2269
        // which loop follows the walk, and whether the backend is asked to run it (K20 raw reads; K21 HiFi reads and -fast, which
        // wins over HiFi here as in after_main)
        main.cns_mode = prm.fast ? 2 : prm.read_type == 3 ? 1 : 0;
        main.want_cns = prm.fast ? cns_fast_on_device() : prm.read_type == 3 ? cns_hifi_on_device() : cns_on_device();
        main.min_cov = (int)prm.min_cov;
        main.lq_max_len = lq_max_len;
    }

    void finish_error(unsigned code) {
        result = Result();
        result.len = code;
        error2 = true;
        phase = PileEngine::DONE;
    }

    void collect(std::vector<AlnJob *> &out) {
        if (phase != PileEngine::LQ_ROUND || lq.ok) return;
        for (AlnJob &j : jobs) out.push_back(&j);
    }

    void advance() {
        const uint64_t t0 = now_ns();
        const int ph = phase == PileEngine::MAIN ? 0 : phase == PileEngine::EXTRACT || phase == PileEngine::POA ? 1 : lq_iter <= 1 ? 2 : 3;
        if (phase == PileEngine::MAIN) after_main();
        else if (phase == PileEngine::EXTRACT) after_extract();
        else if (phase == PileEngine::POA) after_poa();
        else if (phase == PileEngine::LQ_ROUND) after_lq_round();
        else if (phase == PileEngine::SPLICE) after_splice();
        g_prof.adv_ns[ph] += now_ns() - t0;  // per-thread sums: after main / after extract / after LQ round 1 / after round 2 + splice
    }

    // -- main phase: the device returns the best_pp walk --------------------------------
    // The walk's consensus words and windows from the backend (K20; opt-in, see DESIGN.md section 0a'''''''''): raw reads, not -fast.
    static bool cns_on_device() {
        static const bool on = getenv("NDGPU_CNS_DEVICE") != nullptr && atoi(getenv("NDGPU_CNS_DEVICE")) != 0;
        return on;
    }
    // K21 (opt-in, DESIGN.md section 0a''''''''''): NDGPU_CNS_HIFI=1 -- read type 3, not -fast; NDGPU_CNS_FAST=1 -- -fast, any read type.
    // Independent of NDGPU_CNS_DEVICE, which goes on meaning raw reads alone.
    static bool cns_hifi_on_device() {
        static const bool on = getenv("NDGPU_CNS_HIFI") != nullptr && atoi(getenv("NDGPU_CNS_HIFI")) != 0;
        return on;
    }
    static bool cns_fast_on_device() {
        static const bool on = getenv("NDGPU_CNS_FAST") != nullptr && atoi(getenv("NDGPU_CNS_FAST")) != 0;
        return on;
    }
    void after_main() {
        if (main.cns_ready && main.cns_mode == 2) {  // the backend ran cns_fast's loop and scan: length and identity are ours
            main.cns_ready = false;
            std::string seq;
            seq.swap(main.cns_seq);
            fast_result(main.cns_fast[0], main.cns_fast[1], main.cns_fast[2], std::move(seq));
            phase = PileEngine::DONE;
            return;
        }
        if (main.cns_ready && main.cns_mode == 1) {  // the backend ran cns_kmer's loop: the verdict and the reversal are ours
            std::vector<uint32_t> words, wins;
            words.swap(main.cns_words), wins.swap(main.cns_windows);
            main.cns_ready = false;
            CnsCounts c;
            c.len = main.cns_counts[0], c.lqseq_total_length = main.cns_counts[4];
            n_aligned = main.n_aligned;
            if (!cns_kmer_from_words(words.data(), wins.data(), wins.size() / 2, c)) {
                finish_error(2);
                return;
            }
            to_extract();
            return;
        }
        if (main.cns_ready) {  // the backend ran cns_from_best_score's loop: its words, windows and counters; the verdict is ours
            std::vector<uint32_t> words, wins;
            words.swap(main.cns_words), wins.swap(main.cns_windows);
            main.cns_ready = false;
            CnsCounts c;
            c.len = main.cns_counts[0], c.uncorrected_len = main.cns_counts[1], c.lstrip = main.cns_counts[2], c.rstrip = main.cns_counts[3];
            c.lqseq_total_length = main.cns_counts[4];
            n_aligned = main.n_aligned;
            if (!cns_from_words(words.data(), wins.data(), wins.size() / 2, c)) {
                finish_error(2);
                return;
            }
            to_extract();
            return;
        }
        std::vector<PathStep> path;
        path.swap(main.path);
        if (path.empty()) {  // no column carries a tag (reference: undefined behaviour)
            finish_error(2);
            return;
        }
        if (prm.fast) {
            cns_fast(path);
            phase = PileEngine::DONE;
            return;
        }
        n_aligned = main.n_aligned;
        const bool ok = prm.read_type == 3 ? cns_kmer(path) : cns_from_best_score(path);
        if (!ok) {
            finish_error(2);
            return;
        }
        to_extract();
    }
    // the windows as an extract request (none: straight to the first low-quality-region round)
    void to_extract() {
        lq_iter = 0;
        lq_max_dif_len = 0;
        if (regions.empty()) {
            lq_max_aln_length = 0;
            start_lq_round();
            return;
        }
        extract.slot = main.slot;
        extract.rank = rank_on_device() && prm.read_type != 3;  // (HiFi: its ranking sits behind the phasing: K22, below)
        extract.phase = phase_on_device() && prm.read_type == 3;
        extract.n_aligned = n_aligned;
        extract.regions.resize(regions.size());
        for (size_t i = 0; i < regions.size(); i++) {
            extract.regions[i].start = regions[i].start;
            extract.regions[i].end = regions[i].end;
            extract.regions[i].max_len = lq_max_len;
            extract.regions[i].max_len0 = prm.read_type == 3 ? 10000 : 0;  // DAG_MAX_LENGTH, nextcorrect.c:765
        }
        phase = PileEngine::EXTRACT;
    }

    uint64_t poa_ns_local = 0;
    // The regions' POA problems as backend requests (Backend::run_poa): after_extract ranks and selects as ever and posts a request
    // where it used to call poa_consensus; run_engines offers the requests of all live piles to the backend in one batch; after_poa
    // takes a region's turn up again where the call stood.  What the backend does not take (or declines) is computed here, by
    // poa_consensus.  Off (the default, see DESIGN.md section 0a''): the call stays where it was.
    struct PoaPending {
        size_t region;
        int add_len;       // what the region adds to its pseudo-seed's length for the alignment buffers' bound
        bool check_len;    // check_pseudo_seed_length follows (not in the HiFi path)
    };
    std::vector<PoaReq> poa_reqs;
    std::vector<PoaPending> poa_pending;
    static bool poa_as_request() {
        static const bool on = getenv("NDGPU_POA_DEVICE") != nullptr && atoi(getenv("NDGPU_POA_DEVICE")) != 0;
        return on;
    }
    // The 8-mer ranking of the regions' candidates by the backend, behind its extraction (K14; opt-in, see DESIGN.md section 0a''').
    static bool rank_on_device() {
        static const bool on = getenv("NDGPU_RANK_DEVICE") != nullptr && atoi(getenv("NDGPU_RANK_DEVICE")) != 0;
        return on;
    }
    // The phasing and ranking of a HiFi pile's candidates by the backend, behind its extraction (K22; opt-in, see DESIGN.md section 0a''''''''''').
    static bool phase_on_device() {
        static const bool on = getenv("NDGPU_PHASE_DEVICE") != nullptr && atoi(getenv("NDGPU_PHASE_DEVICE")) != 0;
        return on;
    }
    void post_poa(size_t region, std::vector<std::string> &&in, int add_len, bool check_len) {
        poa_reqs.emplace_back();
        poa_reqs.back().seqs = std::move(in);
        poa_pending.push_back(PoaPending{region, add_len, check_len});
    }
    void collect_poa(std::vector<PoaReq *> &out) {
        if (phase != PileEngine::POA) return;
        for (PoaReq &r : poa_reqs) out.push_back(&r);
    }

    void after_extract() {
        const uint64_t t0 = now_ns();
        poa_ns_local = 0;
        poa_reqs.clear(), poa_pending.clear();
        lq_max_aln_length = prm.read_type == 3 ? lqseqs_from_candidates_kmer() : lqseqs_from_candidates();
        extract.regions.clear();
        const uint64_t t1 = now_ns();
        g_prof.poa_ns += poa_ns_local;
        g_prof.rank_ns += t1 - t0 - poa_ns_local;
        if (!poa_reqs.empty()) {
            phase = PileEngine::POA;
            return;
        }
        start_lq_round();
        g_prof.lqstart_ns += now_ns() - t1;
    }

    void after_poa() {
        const uint64_t t0 = now_ns();
        for (size_t i = 0; i < poa_reqs.size(); i++) {
            PoaReq &rq = poa_reqs[i];
            const PoaPending &pp = poa_pending[i];
            LqRegion &lq = regions[pp.region];
            if (!rq.done) rq.out = poa_consensus(rq.seqs);
            lq.sudoseed.swap(rq.out);
            lq.has_seed = true;
            lq.sudoseed_len = (unsigned)lq.sudoseed.size();
            if (pp.check_len) check_pseudo_seed_length(lq);
            if (pp.add_len + (int)lq.sudoseed_len > lq_max_aln_length) lq_max_aln_length = pp.add_len + (int)lq.sudoseed_len;
        }
        poa_reqs.clear(), poa_pending.clear();
        const uint64_t t1 = now_ns();
        g_prof.poa_ns += t1 - t0;
        start_lq_round();
        g_prof.lqstart_ns += now_ns() - t1;
    }

    // lib/nextcorrect.c:1717-1784.  The loop, the table of lower-case runs and its scan are cns_fast_host (nd_cns.h); length and identity
    // follow here, whoever ran the loop.
    void cns_fast(const std::vector<PathStep> &path) {
        CnsFastOut o;
        cns_fast_host(path.data(), path.size(), (int)prm.min_cov, o);
        fast_result(o.lq_m, o.hq_m, o.lq_total_len, std::move(o.seq));
    }
    void fast_result(uint32_t lq_m, uint32_t hq_m, uint32_t lq_total_len, std::string &&seq) {
        result.len = cns_fast_len(lq_m, hq_m);
        result.identity = cns_fast_identity(lq_total_len, result.len);
        result.seq = std::move(seq);
    }

    // lib/nextcorrect.c:1885-2006.  Returns false for the error_seed(2) outcome.  The loop is cns_windows_host (nd_cns.h); the verdict
    // and reverse_consensus_base follow it here, whoever ran the loop.
    bool cns_from_best_score(const std::vector<PathStep> &path) {
        std::vector<uint32_t> words, flat;
        std::vector<CnsWindow> wins;
        CnsCounts c;
        cns_windows_host(path.data(), path.size(), (int)prm.min_cov, lq_max_len, words, wins, c);
        for (const CnsWindow &w : wins) flat.push_back(w.start), flat.push_back(w.end);
        return cns_from_words(words.data(), flat.data(), wins.size(), c);
    }
    // words: pos << 8 | char in walk order; wins: (start, end) pairs in emission order
    bool cns_from_words(const uint32_t *words, const uint32_t *wins, size_t n_wins, const CnsCounts &c) {
        cns = CnsData();
        regions.clear();
        cns.len = c.len, cns.uncorrected_len = c.uncorrected_len, cns.lstrip = c.lstrip, cns.rstrip = c.rstrip;
        if (!cns_verdict(c, prm.min_error_corrected_ratio)) return false;
        cns.bases.resize(c.len);
        for (uint32_t p = 0; p < c.len; p++) cns.bases[c.len - 1 - p] = CnsBase{words[p] >> 8, (char)(words[p] & 0xffu)};  // reverse_consensus_base
        regions.resize(n_wins);
        for (size_t i = 0; i < n_wins; i++) regions[i].start = wins[2 * i], regions[i].end = wins[2 * i + 1];
        return true;
    }

    // HiFi backtrack + LQ windows: lib/nextcorrect.c:1786-1883.  The loop is cns_kmer_host (nd_cns.h); the verdict and
    // reverse_consensus_base follow it here, whoever ran the loop.
    bool cns_kmer(const std::vector<PathStep> &path) {
        const char *seed = !seq_ptr.empty() ? seq_ptr[0] : (seed_copy.empty() ? nullptr : seed_copy.c_str());
        if (!seed) {
            fprintf(stderr, "[ndgpu] HiFi consensus needs the seed sequence on the host\n");
            return false;
        }
        std::vector<uint32_t> words, flat;
        std::vector<CnsWindow> wins;
        CnsCounts c;
        cns_kmer_host(path.data(), path.size(), CnsSeedAscii{seed}, (int)prm.min_cov, words, wins, c);
        for (const CnsWindow &w : wins) flat.push_back(w.start), flat.push_back(w.end);
        return cns_kmer_from_words(words.data(), flat.data(), wins.size(), c);
    }
    bool cns_kmer_from_words(const uint32_t *words, const uint32_t *wins, size_t n_wins, const CnsCounts &c) {
        cns = CnsData();
        regions.clear();
        cns.len = c.len;  // uncorrected_len, lstrip, rstrip stay 0 in this variant
        if (!cns_kmer_verdict(c, prm.min_error_corrected_ratio)) {
            // (the reference leaves the loop's bases and windows behind the refusal; nothing reads them)
            return false;
        }
        cns.bases.resize(c.len);
        for (uint32_t p = 0; p < c.len; p++) cns.bases[c.len - 1 - p] = CnsBase{words[p] >> 8, (char)(words[p] & 0xffu)};  // reverse_consensus_base
        regions.resize(n_wins);
        for (size_t i = 0; i < n_wins; i++) regions[i].start = wins[2 * i], regions[i].end = wins[2 * i + 1];
        return true;
    }

    // HiFi: generate_lqseqs_from_tags_kmer, lib/nextcorrect.c:740-1008, on the extracted candidates: lay them out, phase and rank them
    // (hifi_phase_host of nd_phase.h, lines 787-948 with the helpers of 512-737 -- or the records the backend left where the pile asked
    // for them: K22), apply the records, then the selection loop and the POA hand-over as ever.
    // What applying a record relies on: perm is a permutation of the region's candidates, kind, n and seed_pos lie inside them.
    static bool phase_record_ok(const PhaseRecord &r, size_t n_cand) {
        if (n_cand > (size_t)kPhaseCanMax || r.kind > kPhaseRanked) return false;
        if (r.kind == kPhaseEmpty) return n_cand == 0;
        uint64_t seen = 0;
        for (size_t p = 0; p < n_cand; p++) {
            if (r.perm[p] >= n_cand || (seen >> r.perm[p]) & 1u) return false;
            seen |= 1ull << r.perm[p];
        }
        if (r.kind == kPhaseSeed) return r.seed_pos < n_cand && r.n == -2;
        if (r.kind == kPhaseRanked) return r.n >= 1 && (size_t)r.n <= n_cand;
        return r.n == 0;
    }
    int lqseqs_from_candidates_kmer() {
        int max_aln_length = 0, max_aln_lqseq_len = 0;
        int k, j;
        bool phased = extract.phase;
        size_t n_cands = 0;
        for (size_t ri = 0; ri < regions.size(); ri++) {
            LqRegion &lq = regions[ri];
            RegionReq &rq = extract.regions[ri];
            lq.len = 0;
            lq.seqs.clear();
            lq.has_seed = false;
            for (size_t c = 0; c < rq.cands.size(); c++) {
                LqSeq q;
                q.len = (uint16_t)rq.cands[c].size();
                q.order = rq.cand_rank[c];  // source read
                q.kscore = 0;
                if ((int)q.len > max_aln_lqseq_len) max_aln_lqseq_len = q.len;
                q.seq = std::move(rq.cands[c]);
                lq.seqs.push_back(std::move(q));
                lq.len++;
            }
            n_cands += lq.seqs.size();
            phased = phased && rq.phased;
        }
        std::vector<PhaseRecord> recs(regions.size());
        if (phased) {
            for (size_t ri = 0; ri < regions.size() && phased; ri++) {
                recs[ri] = extract.regions[ri].phase;
                phased = phase_record_ok(recs[ri], regions[ri].seqs.size());
            }
            if (!phased) fprintf(stderr, "[ndgpu] a backend's phasing record does not fit its region: the pile takes the host rule\n");
        }
        if (!phased) {
            std::vector<const char *> ptr(n_cands);
            std::vector<uint16_t> len(n_cands), src(n_cands);
            std::vector<PhaseRegionIn> in(regions.size());
            size_t at = 0;
            for (size_t ri = 0; ri < regions.size(); ri++) {
                const LqRegion &lq = regions[ri];
                in[ri] = PhaseRegionIn{lq.start, lq.end, lq.len, ptr.data() + at, len.data() + at, src.data() + at};
                for (const LqSeq &q : lq.seqs) ptr[at] = q.seq.data(), len[at] = q.len, src[at] = q.order, at++;
            }
            PhasePileOut pile;
            hifi_phase_host(n_aligned, in.data(), in.size(), recs.data(), pile);
        }
        for (size_t ri = 0; ri < regions.size(); ri++) {
            LqRegion &lq = regions[ri];
            const PhaseRecord &rec = recs[ri];
            if (rec.kind == kPhaseEmpty) continue;
            {  // lq.seqs as the rule left them
                std::vector<LqSeq> moved(lq.seqs.size());
                for (size_t p = 0; p < moved.size(); p++) {
                    moved[p] = std::move(lq.seqs[rec.perm[p]]);
                    moved[p].kscore = rec.kscore[p];
                }
                lq.seqs.swap(moved);
            }
            lq.indexs = rec.indexs;
            if (rec.kind == kPhaseDropped) {
                lq.len = 0;
                continue;
            }
            if (rec.kind == kPhaseSeed) {
                const LqSeq &q = lq.seqs[rec.seed_pos];
                lq.sudoseed = q.seq;
                lq.sudoseed_len = q.len;
                lq.has_seed = true;
                if (rec.lower)
                    for (char &ch : lq.sudoseed) ch = (char)tolower(ch);
                lq.len = -2;
            } else {
                lq.len = rec.n;
                unsigned klastscore, kmaxscore;
                unsigned kmaxlen = lq.seqs[0].len;
                klastscore = kmaxscore = lq.seqs[0].kscore;
                for (k = j = 0; j < lq.len; j++) {
                    const unsigned ks = lq.seqs[j].kscore;
                    if (ks * 10 < kmaxscore || j >= kLqSeqMax || ks * 2 < klastscore) break;
                    klastscore = ks;
                    if (j < kKmerMaxSeq && ks > kmaxscore * 0.8 && lq.seqs[j].len > kmaxlen) {
                        kmaxlen = lq.seqs[j].len;
                        k = j;
                    }
                }
                lq.indexs = 0;
                lq.indexe = (uint8_t)(kmaxlen > (unsigned)kLqRevLen && j > 6 ? 5 : j - 1);
                if ((int)lq.indexe - (int)lq.indexs <= 1 || (lq.seqs[0].len > 20000 && lq.len < kLqCanMax / 3)) {
                    lq.len = 0;
                    continue;
                }
                j = lq.indexs;
                if (lq.seqs[0].len < 3000) k = j + 6 < lq.indexe ? 6 : lq.indexe - j + 1;
                else k = j + 2 < lq.indexe ? 2 : lq.indexe - j + 1;
                if (lq.seqs[0].len < 20000) {
                    std::vector<std::string> in;
                    for (int x = 0; x < k; x++) in.push_back(lq.seqs[j + x].seq);
                    if (poa_as_request()) {  // (the rest of this region's turn: after_poa)
                        post_poa(ri, std::move(in), max_aln_lqseq_len, false);
                        continue;
                    }
                    { const uint64_t tp = now_ns(); lq.sudoseed = poa_consensus(in); poa_ns_local += now_ns() - tp; }
                } else lq.sudoseed = lq.seqs[0].seq;
                lq.has_seed = true;
                lq.sudoseed_len = (unsigned)lq.sudoseed.size();
            }
            if (max_aln_lqseq_len + (int)lq.sudoseed_len > max_aln_length) max_aln_length = max_aln_lqseq_len + (int)lq.sudoseed_len;
        }
        return max_aln_length;
    }

    // lib/nextcorrect.c:356-510 with the candidate strings (lines 373-404) already
    // gathered by the backend
    int lqseqs_from_candidates() {
        int max_aln_length = 0;
        for (size_t ri = 0; ri < regions.size(); ri++) {
            LqRegion &lq = regions[ri];
            RegionReq &rq = extract.regions[ri];
            int max_len_here = 0;
            const int large_seq = (int)rq.n_large;
            lq.len = 0;
            lq.seqs.clear();
            lq.has_seed = false;
            for (std::string &s : rq.cands) {
                LqSeq q;
                q.len = (uint16_t)s.size();
                q.order = (uint16_t)lq.len;
                if ((int)s.size() > max_len_here) max_len_here = (int)s.size();
                q.seq = std::move(s);
                lq.seqs.push_back(std::move(q));
                lq.len++;
            }
            if ((float)large_seq / (lq.len + large_seq) > 1.0 / 3 || lq.len <= 4 || (prm.split && lq.len < 10)) {
                lq.len = 0;
                continue;
            }
            // the ranking: the backend's (K14 behind K11, where the region carries one) or the host routine's -- either way as
            // (order, kscore), in which the candidates are then laid out
            unsigned klastscore, kmaxscore, kmaxlen, kminlen;
            {
                uint8_t order_h[kLqCanMax];
                uint16_t kscore_h[kLqCanMax];
                const uint8_t *order = rq.rank_order;
                const uint16_t *kscore = rq.rank_kscore;
                if (!rq.ranked) {
                    const char *ptr[kLqCanMax];
                    uint16_t len[kLqCanMax];
                    int tail = 0;
                    for (int j = 0; j < lq.len; j++) ptr[j] = lq.seqs[j].seq.data(), len[j] = lq.seqs[j].len;
                    lq_rank_host(ptr, len, lq.len, order_h, kscore_h, &tail);
                    order = order_h, kscore = kscore_h;
                }
                std::vector<LqSeq> ranked((size_t)lq.len);
                for (int j = 0; j < lq.len; j++) {
                    ranked[j] = std::move(lq.seqs[order[j]]);
                    ranked[j].kscore = kscore[j];
                }
                lq.seqs.swap(ranked);
            }
            kminlen = kmaxlen = lq.seqs[0].len;
            klastscore = kmaxscore = lq.seqs[0].kscore;
            int j, k;
            for (k = j = 0; j < lq.len; j++) {
                const unsigned ks = lq.seqs[j].kscore;
                if (ks * 10 < kmaxscore || j >= kLqSeqMax || ks * 2 < klastscore ||
                    (j > 4 && kmaxlen > 200 && ks < kmaxscore * 0.6 && lq.seqs[j].len < kminlen * 0.8))
                    break;
                klastscore = ks;
                if (j < kKmerMaxSeq && ks > kmaxscore * 0.8) {
                    if (lq.seqs[j].len > kmaxlen) kmaxlen = lq.seqs[j].len;
                    else if (lq.seqs[j].len < kminlen) kminlen = lq.seqs[j].len;
                }
            }
            lq.indexs = 0;
            lq.indexe = (uint8_t)(kmaxlen > (unsigned)kLqRevLen && j > 6 ? 5 : j - 1);
            if ((int)lq.indexe - (int)lq.indexs <= 3) {
                lq.len = 0;
                continue;
            }
            j = lq.indexs;
            if (lq.seqs[0].len < 3000) k = j + 6 < lq.indexe ? 6 : lq.indexe - j + 1;
            else k = j + 2 < lq.indexe ? 2 : lq.indexe - j + 1;
            {
                std::vector<std::string> in;
                for (int x = 0; x < k; x++) in.push_back(lq.seqs[j + x].seq);
                if (poa_as_request()) {  // (the rest of this region's turn: after_poa)
                    post_poa(ri, std::move(in), max_len_here, true);
                    continue;
                }
                { const uint64_t tp = now_ns(); lq.sudoseed = poa_consensus(in); poa_ns_local += now_ns() - tp; }
            }
            lq.has_seed = true;
            lq.sudoseed_len = (unsigned)lq.sudoseed.size();
            check_pseudo_seed_length(lq);
            if (max_len_here + (int)lq.sudoseed_len > max_aln_length) max_aln_length = max_len_here + (int)lq.sudoseed_len;
        }
        return max_aln_length;
    }

    // a POA consensus of more than 500 bases that is over a tenth longer than its candidates' trimmed mean gives way to one of them
    void check_pseudo_seed_length(LqRegion &lq) {
        int j, k;
        {
            if (lq.sudoseed_len > 500) {
                int kmax, kmin;
                k = kmax = kmin = lq.seqs[lq.indexs].len;
                for (j = lq.indexs + 1; j <= lq.indexe && j <= lq.indexs + 4; j++) {
                    k += lq.seqs[j].len;
                    if (lq.seqs[j].len > kmax) kmax = lq.seqs[j].len;
                    else if (lq.seqs[j].len < kmin) kmin = lq.seqs[j].len;
                }
                k = kmax != kmin ? (k - kmax - kmin) / (j - lq.indexs - 2) : k / (j - lq.indexs);
                if (lq.sudoseed_len > (unsigned)(k + k / 10)) {
                    for (kmin = k, k = lq.indexs; k < j; k++)
                        if (lq.seqs[k].len != kmax && lq.seqs[k].len >= kmin) break;
                    if (j == k)
                        for (k = 0; k < lq.len && lq.seqs[k].order; k++) {}
                    if (k >= lq.len) k = 0;  // unreachable: order 0 always survives
                    lq.sudoseed = lq.seqs[k].seq;
                    lq.sudoseed_len = lq.seqs[k].len;
                }
            }
        }
    }

    // -- low-quality-region rounds (lib/nextcorrect.c:1671-1715, 1538-1669) ----------
    void start_lq_round() {
        lq_iter++;
        lq_max_aln_length += lq_max_dif_len;
        jobs.clear();
        lq_slots.clear();
        lq.pieces.clear();
        lq.lqc.clear();
        lq.ok = false;
        const int count = (int)regions.size();
        for (int i = 0; i < kLqSeqMax; i++) {
            for (int j = count - 1; j >= 0; j--) {
                LqRegion &r = regions[j];
                if (r.len <= 0) continue;
                const int sl = (int)r.sudoseed_len;
                const bool past = i + r.indexs > r.indexe;
                const int ql = past ? sl : r.seqs[i + r.indexs].len;
                LqSlot slot{i, j, -1};
                if (!(past || (i && (ql < sl * 0.5 || ql > sl * 1.3)))) {
                    AlnJob job;
                    job.q = r.seqs[i + r.indexs].seq.c_str();
                    job.q_len = ql;
                    job.t = r.sudoseed.c_str();
                    job.t_len = sl;
                    job.hq = prm.read_type == 3;
                    LqSeq &qs = r.seqs[i + r.indexs];
                    if (qs.packed.empty() && ql > 0) {
                        qs.packed.resize(((size_t)ql + 15) / 16);
                        if (!pack_2bit_lsb(qs.packed.data(), job.q, (size_t)ql)) qs.packed.clear();  // (bytes outside ACGT: packed per call, reported there)
                    }
                    job.q_words = qs.packed.empty() ? nullptr : qs.packed.data();
                    slot.job = (int)jobs.size();
                    jobs.push_back(std::move(job));
                }
                lq_slots.push_back(slot);
                lq.pieces.push_back(LqRound::Piece{slot.job, (unsigned)sl});
            }
        }
        lq.jobs = &jobs;
        lq.n_regions = (unsigned)(lq.pieces.size() / kLqSeqMax);
        lq.factor = prm.read_type == 3 ? 4 : 2;
        lq.qv_factor = prm.read_type == 3 ? 2 : 5;
        phase = PileEngine::LQ_ROUND;
        if (jobs.empty()) after_lq_round();  // nothing to align: still run the round
    }

    void after_lq_round() {
        if (lq.ok) {  // the device ran the round (K12): its walk is the string the host path builds below
            jobs.clear();
            lq_slots.clear();
            std::string lqc;
            lqc.swap(lq.lqc);
            lq.ok = false;
            rewrite_pseudo_seeds(lqc);
            return;
        }
        // generate_consensus_trimed: build the 30 linked rows, second MSA, backtrack
        const int count = (int)regions.size();
        size_t link_len = 1;
        for (int j = count - 1; j >= 0; j--)
            if (regions[j].len > 0) link_len += regions[j].sudoseed_len + 1;
        Msa msa(link_len);
        std::vector<TagList> rows(kLqSeqMax);
        size_t slot_at = 0;
        std::string t_str, q_str;
        for (int i = 0; i < kLqSeqMax; i++) {
            t_str.clear();
            q_str.clear();
            for (int j = count - 1; j >= 0; j--) {
                LqRegion &r = regions[j];
                if (r.len <= 0) continue;
                const LqSlot &slot = lq_slots[slot_at++];
                const int sl = (int)r.sudoseed_len;
                t_str.push_back('N');
                q_str.push_back('N');
                const AlnJob *job = slot.job >= 0 ? &jobs[slot.job] : nullptr;
                if (job && job->status == ALN_OK && job->ops.size() > 2) {
                    const char *q = job->q, *t = job->t;
                    int qi = 0, ti = 0;
                    for (uint8_t op : job->ops) {
                        if (op == OP_MATCH) { t_str.push_back(t[ti++]); q_str.push_back(q[qi++]); }
                        else if (op == OP_QONLY) { t_str.push_back('-'); q_str.push_back(q[qi++]); }
                        else { t_str.push_back(t[ti++]); q_str.push_back('-'); }
                    }
                    int tl = job->t_used, ql = job->q_used;
                    while (tl < sl) { t_str.push_back(r.sudoseed[tl++]); q_str.push_back('-'); }
                    int delta = 0;
                    const LqSeq &qs = r.seqs[slot.i + r.indexs];
                    while (ql < qs.len && delta++ < 250) { q_str.push_back(qs.seq[ql++]); t_str.push_back('-'); }
                } else {
                    t_str.append((size_t)sl, 'M');
                    q_str.append((size_t)sl, 'M');
                }
            }
            t_str.push_back('N');
            q_str.push_back('N');
            tags_from_strings(t_str, q_str, 0, rows[i], msa);
        }
        jobs.clear();
        lq_slots.clear();

        // get_lqseqs_from_align_tags (nextcorrect.c:1250-1338)
        msa.allocate();
        msa.count_links(rows);
        rows.clear();
        Pos cur = msa.score_lq(prm.read_type == 3 ? 4 : 2);
        const int min_qv_factor = prm.read_type == 3 ? 2 : 5;
        std::string lqc;
        while (true) {
            if (cur.b != 4) {
                const Cell &c = msa.cell(cur.t, cur.d, cur.b);
                const char ch = (char)kIntToBase[cur.b];
                lqc.push_back((int)c.best_link * min_qv_factor > (int)msa.coverage[cur.t] || ch == 'N' ? ch : (char)tolower(ch));
            }
            const Cell &c = msa.cell(cur.t, cur.d, cur.b);
            cur = Pos{c.best_t, c.best_d, c.best_b};
            if (cur.t == -1) break;
        }
        rewrite_pseudo_seeds(lqc);
    }

    // iterate_generate_consensus_trimed body (nextcorrect.c:1684-1710): the walk's characters (origin first) become the
    // regions' new pseudo-seeds; then the second round, or the splice
    void rewrite_pseudo_seeds(const std::string &lqc) {
        const int count = (int)regions.size();
        int j = count;
        int psed_len = 0;
        lq_max_dif_len = 0;
        for (size_t k = lqc.size(); k; k--) {
            const char ch = lqc[k - 1];
            if (ch != 'N') {
                if (j < 0 || j >= count) { finish_error(2); return; }  // reference: out-of-bounds write
                LqRegion &r = regions[j];
                if (r.sudoseed.size() <= r.sudoseed_len) r.sudoseed.resize(r.sudoseed_len + 1);
                if (ch < 'a') r.sudoseed[r.sudoseed_len++] = ch;
                else {
                    r.sudoseed[r.sudoseed_len++] = (char)toupper(ch);
                    r.lqcount++;
                }
            } else {
                if (j != count && j >= 0) {
                    LqRegion &r = regions[j];
                    r.sudoseed.resize(r.sudoseed_len);
                    if ((int)r.sudoseed_len > psed_len + lq_max_dif_len) lq_max_dif_len = (int)r.sudoseed_len - psed_len;
                    if (r.lqcount > r.sudoseed_len * 4 / 5) r.len = -1;
                }
                j--;
                while (j >= 0 && regions[j].len <= 0) j--;
                if (j < 0) continue;
                psed_len = (int)regions[j].sudoseed_len;
                regions[j].sudoseed_len = regions[j].lqcount = 0;
            }
        }
        if (lq_iter < 2) {
            start_lq_round();
            return;
        }
        if (splice_on_device()) post_splice();
        else splice();
    }

    // K24 (opt-in): NDGPU_SPLICE_DEVICE=1 -- the splice goes to the backend as a request, whatever the read type.
    static bool splice_on_device() {
        static const bool on = getenv("NDGPU_SPLICE_DEVICE") != nullptr && atoi(getenv("NDGPU_SPLICE_DEVICE")) != 0;
        return on;
    }
    // The request: the words go up with it (the batch's own copy of K20's words is gone by now: its slot is reused by the next
    // launch of the main phase), the regions point into this pile's.
    void post_splice() {
        sp_words.resize(cns.len);
        for (unsigned i = 0; i < cns.len; i++) sp_words[i] = cns.bases[i].pos << 8 | (unsigned char)cns.bases[i].base;
        fill_splice_regions();
        sp_req = SpliceReq();
        sp_req.words = sp_words.data(), sp_req.len = cns.len, sp_req.lstrip = cns.lstrip, sp_req.rstrip = cns.rstrip;
        sp_req.regions = sp_regions.data(), sp_req.n_regions = sp_regions.size(), sp_req.hifi = prm.read_type == 3;
        phase = PileEngine::SPLICE;
    }
    // What came back: the host contributes the identity alone (a declined request, or a backend without the entry: splice()).
    void after_splice() {
        if (!sp_req.done) {
            splice();
            return;
        }
        const bool empty2 = sp_req.code == 2u;
        result.identity = splice_identity(sp_req.lq_total_len, splice_len(sp_req.lq_m, sp_req.hq_m, empty2), empty2);
        result.len = sp_req.code ? sp_req.code : (unsigned)sp_req.seq.size();
        result.seq.swap(sp_req.seq);
        std::vector<uint32_t>().swap(sp_words);
        phase = PileEngine::DONE;
    }
    void fill_splice_regions() {
        sp_regions.resize(regions.size());
        for (size_t k = 0; k < regions.size(); k++) {
            const LqRegion &r = regions[k];
            sp_regions[k].start = r.start, sp_regions[k].end = r.end, sp_regions[k].len = r.len;
            sp_regions[k].sudoseed_len = r.sudoseed_len, sp_regions[k].sudoseed = r.sudoseed.data();
        }
    }

    // update_consensus_trimed (lib/nextcorrect.c:1365-1482) and trim_terminal_ssr (:2008-2128): the rule is nd_splice.h's
    void splice() {
        struct Words {
            const CnsBase *b;
            uint32_t operator[](size_t i) const { return b[i].pos << 8 | (unsigned char)b[i].base; }
        };
        fill_splice_regions();
        SpliceAnswer a;
        splice_answer_host(Words{cns.bases.data()}, cns.len, cns.lstrip, cns.rstrip, sp_regions.data(), sp_regions.size(), prm.read_type == 3, a);
        result.len = a.len;
        result.identity = a.identity;
        result.seq.swap(a.seq);
        phase = PileEngine::DONE;
    }

    ConsensusTrimed *take() {
        if (error2 || result.len <= 4) {
            ConsensusTrimed *c = make_error_seed(result.len);
            c->identity = result.identity;
            if (!error2 && result.len == 4) memcpy(c->seq, result.seq.data(), std::min<size_t>(4, result.seq.size()));
            return c;
        }
        ConsensusTrimed *c = (ConsensusTrimed *)malloc(sizeof(ConsensusTrimed));
        c->len = result.len;
        c->identity = result.identity;
        c->seq = (char *)malloc((size_t)result.len + 1);
        memcpy(c->seq, result.seq.data(), result.len);
        c->seq[result.len] = '\0';
        return c;
    }
};

PileEngine::PileEngine(const char *const *seqs, const unsigned *aln_start, const unsigned *aln_end, unsigned seq_count,
                       const CorrectParams &prm)
    : impl_(new PileImpl(seqs, nullptr, nullptr, aln_start, aln_end, seq_count, prm, nullptr)) {}
PileEngine::PileEngine(const unsigned *seq_len, const int64_t *dev_off, const unsigned *aln_start,
                       const unsigned *aln_end, unsigned seq_count, const CorrectParams &prm, const char *seed)
    : impl_(new PileImpl(nullptr, seq_len, dev_off, aln_start, aln_end, seq_count, prm, seed)) {}
PileEngine::~PileEngine() { delete impl_; }
PileEngine::Phase PileEngine::phase() const { return impl_->phase; }
MainPile *PileEngine::main_request() { return &impl_->main; }
ExtractPile *PileEngine::extract_request() { return &impl_->extract; }
void PileEngine::collect_jobs(std::vector<AlnJob *> &out) { impl_->collect(out); }
LqRound *PileEngine::lq_request() { return impl_->phase == LQ_ROUND && !impl_->jobs.empty() ? &impl_->lq : nullptr; }
void PileEngine::collect_poa(std::vector<PoaReq *> &out) { impl_->collect_poa(out); }
SpliceReq *PileEngine::splice_request() { return &impl_->sp_req; }
void PileEngine::advance() { impl_->advance(); }
ConsensusTrimed *PileEngine::take_result() { return impl_->take(); }

namespace {
template <typename F>
void parallel_for(size_t n, int threads, F f) {
    if (threads <= 1 || n <= 1) {
        for (size_t i = 0; i < n; i++) f(i);
        return;
    }
    std::atomic<size_t> next(0);
    std::vector<std::thread> pool;
    const int nt = (int)std::min<size_t>((size_t)threads, n);
    for (int t = 0; t < nt; t++)
        pool.emplace_back([&] {
            for (;;) {
                size_t i = next.fetch_add(1);
                if (i >= n) break;
                f(i);
            }
        });
    for (auto &th : pool) th.join();
}
}  // namespace

HostProf g_prof;

bool pack_2bit_lsb(uint32_t *out, const char *s, size_t n) {
    static const struct Lut {
        uint8_t v[256];
        Lut() {
            memset(v, 0xff, sizeof(v));
            v['A'] = 0, v['C'] = 1, v['G'] = 2, v['T'] = 3;  // lib/bseq.c:11-20
        }
    } lut;
    unsigned bad = 0;
    size_t i = 0, w = 0;
    for (; i + 16 <= n; w++, i += 16) {
        uint32_t acc = 0;
        for (int b = 0; b < 16; b++) {
            const uint8_t c = lut.v[(unsigned char)s[i + b]];
            bad |= c;
            acc |= (uint32_t)(c & 3u) << (2 * b);
        }
        out[w] = acc;
    }
    if (i < n) {
        uint32_t acc = 0;
        for (int b = 0; i + b < n; b++) {
            const uint8_t c = lut.v[(unsigned char)s[i + b]];
            bad |= c;
            acc |= (uint32_t)(c & 3u) << (2 * b);
        }
        out[w] = acc;
    }
    return (bad & 0x80u) == 0;
}

int effective_cpus() {
    static const int n = [] {
        int hw = (int)std::max(1u, std::thread::hardware_concurrency());
        cpu_set_t set;
        if (sched_getaffinity(0, sizeof(set), &set) == 0) {
            const int a = CPU_COUNT(&set);
            if (a > 0 && a < hw) hw = a;
        }
        auto from_quota = [&](double quota, double period) {
            if (quota > 0 && period > 0) {
                const int q = (int)std::ceil(quota / period - 1e-9);
                if (q >= 1 && q < hw) hw = q;
            }
        };
        if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {  // cgroup v2: "max 100000" or "1600000 100000"
            char a[64] = {0};
            double period = 0;
            if (fscanf(f, "%63s %lf", a, &period) == 2 && strcmp(a, "max") != 0) from_quota(atof(a), period);
            fclose(f);
        } else {
            double quota = -1, period = 0;
            if (FILE *q = fopen("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "r")) {
                if (fscanf(q, "%lf", &quota) != 1) quota = -1;
                fclose(q);
            }
            if (FILE *q = fopen("/sys/fs/cgroup/cpu/cpu.cfs_period_us", "r")) {
                if (fscanf(q, "%lf", &period) != 1) period = 0;
                fclose(q);
            }
            from_quota(quota, period);
        }
        if (const char *e = getenv("NDGPU_HOST_CPUS")) hw = std::max(1, atoi(e));  // (override)
        return hw;
    }();
    return n;
}

static std::atomic<int> g_cores_total(0), g_cores_used(0);
void CoreGovernor::set_total(int total) { g_cores_total.store(total < 0 ? 0 : total); }
int CoreGovernor::acquire(int base) {
    if (base < 1) base = 1;
    const int total = g_cores_total.load();
    int used = g_cores_used.load();
    for (;;) {
        int grant = total - used;
        if (grant < base) grant = base;
        static const int cap_mul = getenv("NDGPU_GOV_CAP") ? std::max(1, atoi(getenv("NDGPU_GOV_CAP"))) : 4;
        if (grant > cap_mul * base) grant = cap_mul * base;  // thread start-up and allocator contention eat the gain beyond this
        if (g_cores_used.compare_exchange_weak(used, used + grant)) return grant;
    }
}
void CoreGovernor::release(int granted) { g_cores_used.fetch_sub(granted); }

static inline uint64_t now_ns() {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
               std::chrono::steady_clock::now().time_since_epoch())
        .count();
}

void run_engines(PileEngine **eng, size_t n, Backend &be, int threads) {
    std::vector<MainPile *> mains;
    std::vector<ExtractPile *> extracts;
    std::vector<AlnJob *> jobs;
    std::vector<LqRound *> lqs;
    std::vector<PoaReq *> poas;
    std::vector<SpliceReq *> splices;
    std::vector<size_t> live, in_lq;
    for (;;) {
        mains.clear();
        extracts.clear();
        jobs.clear();
        lqs.clear();
        poas.clear();
        splices.clear();
        live.clear();
        in_lq.clear();
        for (size_t i = 0; i < n; i++) {
            switch (eng[i]->phase()) {
                case PileEngine::MAIN: mains.push_back(eng[i]->main_request()); break;
                case PileEngine::EXTRACT: extracts.push_back(eng[i]->extract_request()); break;
                case PileEngine::POA: eng[i]->collect_poa(poas); break;
                case PileEngine::SPLICE: splices.push_back(eng[i]->splice_request()); break;
                case PileEngine::LQ_ROUND:
                    in_lq.push_back(i);
                    if (LqRound *r = eng[i]->lq_request()) lqs.push_back(r);
                    break;
                default: continue;
            }
            live.push_back(i);
        }
        if (live.empty()) break;
        uint64_t t0 = now_ns();
        if (!mains.empty()) be.run_main(mains.data(), mains.size());
        uint64_t t1 = now_ns();
        if (!extracts.empty()) be.run_extract(extracts.data(), extracts.size());
        // the regions' POA problems: one batch on the backend where it offers that; what it does not take is computed in advance()
        if (!poas.empty()) (void)be.run_poa(poas.data(), poas.size());
        uint64_t t2 = now_ns();
        // low-quality-region rounds: whole rounds on the backend where it offers that; what it does not take (or declines)
        // goes the host way -- the alignments as a batch, the second MSA in the engine
        if (!lqs.empty()) (void)be.run_lq(lqs.data(), lqs.size());
        for (size_t i : in_lq) eng[i]->collect_jobs(jobs);
        if (!jobs.empty()) be.run_align(jobs.data(), jobs.size());
        // the piles behind their last LQ round: the splices as one batch where the backend offers that; the rest is computed in advance()
        if (!splices.empty()) (void)be.run_splice(splices.data(), splices.size());
        uint64_t t3 = now_ns();
        {
            CoreLease lease(threads);
            parallel_for(live.size(), lease.n, [&](size_t k) { eng[live[k]]->advance(); });
        }
        uint64_t t4 = now_ns();
        g_prof.main_ns += t1 - t0;
        g_prof.extract_ns += t2 - t1;
        g_prof.align_ns += t3 - t2;
        g_prof.advance_ns += t4 - t3;
        g_prof.jobs += jobs.size();
        static const bool trace = getenv("NDGPU_TRACE") != nullptr;
        if (trace)  // one line per round of a sub-batch: which phases ran, on how many piles / jobs, and when (ms)
            fprintf(stderr, "[ndgpu trace] be %p piles %zu | main %zu [%.1f %.1f] extract %zu [%.1f] align %zu [%.1f] advance [%.1f]\n",
                    (void *)&be, n, mains.size(), t0 * 1e-6, t1 * 1e-6, extracts.size(), t2 * 1e-6, jobs.size(), t3 * 1e-6, t4 * 1e-6);
    }
    be.end_batch();
}

}  // namespace ndgpu
