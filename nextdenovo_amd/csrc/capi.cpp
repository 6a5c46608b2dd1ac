// C ABI of the engine (include/ndgpu_nextcorrect.h).
#include <hip/hip_runtime_api.h>
#include <cerrno>
#include <sys/uio.h>
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <chrono>
#include <functional>
#include <mutex>
#include <thread>
#include <vector>

#include "../../include/ndgpu_nextcorrect.h"
#include "nd_host.h"
#include "nd_cns.h"
#include "nd_runtime.h"
#include "nd_subplan.h"

using namespace ndgpu;

namespace {

CorrectParams make_params(unsigned max_mem_len, unsigned min_len_aln, unsigned max_cov_aln, unsigned min_cov,
                          unsigned lqseq_max_length, float ratio, unsigned split, unsigned fast, int read_type) {
    CorrectParams p;
    p.max_mem_len = max_mem_len;
    p.min_len_aln = min_len_aln;
    p.max_cov_aln = max_cov_aln;
    p.min_cov = min_cov;
    p.lqseq_max_length = lqseq_max_length;
    p.min_error_corrected_ratio = ratio;
    p.split = split;
    p.fast = fast;
    p.read_type = read_type;
    return p;
}

void run_single_alignment(char *q, int q_len, char *t, int t_len, alignment *a, int hq) {
    AlnJob job;
    job.q = q;
    job.q_len = q_len;
    job.t = t;
    job.t_len = t_len;
    job.hq = hq;
    AlnJob *jp = &job;
    {
        HipBackend be;
        be.run_align(&jp, 1);
    }
    if (job.status == ALN_NONE) return;  // reference leaves *align_rtn untouched (lib/align.c:440-560)
    a->aln_t_e = a->aln_t_s + (unsigned)job.t_used - 1;
    a->aln_t_len = (unsigned)job.t_used;
    a->aln_q_len = (unsigned)job.q_used;
    size_t n = job.ops.size();
    int qi, ti;
    if (job.status == ALN_GAP_ABORT) {
        // reference: aln_len = 2 with the last two alignment columns (lib/align.c:542-556)
        qi = job.q_used;
        ti = job.t_used;
        for (size_t c = n; c-- > 0;) {
            if (job.ops[c] != OP_TONLY) qi--;
            if (job.ops[c] != OP_QONLY) ti--;
        }
    } else {
        qi = ti = 0;
    }
    for (size_t c = 0; c < n; c++) {
        const uint8_t op = job.ops[c];
        a->t_aln_str[c] = op == OP_QONLY ? '-' : t[ti++];
        a->q_aln_str[c] = op == OP_TONLY ? '-' : q[qi++];
    }
    a->t_aln_str[n] = a->q_aln_str[n] = '\0';
    a->aln_len = (unsigned)n;
}

}  // namespace

namespace {
std::mutex g_reap_mu;
std::vector<std::thread> g_reapers;
void join_reapers() {
    std::vector<std::thread> v;
    {
        std::lock_guard<std::mutex> lock(g_reap_mu);
        v.swap(g_reapers);
    }
    for (auto &t : v) t.join();
}
struct ReaperAtExit {
    ~ReaperAtExit() { join_reapers(); }
} g_reaper_at_exit;
}  // namespace

namespace {

// Every record must name reads of this DB and windows inside them (a sorted.ovl written against other .idx files would otherwise
// index the host tables and the device pool out of bounds): -2, nothing is computed
int validate_records(const ReadDb &db, int n_piles, const uint32_t *recs, const uint64_t *pile_off) {
    for (int i = 0; i < n_piles; i++) {
        if (pile_off[i + 1] < pile_off[i]) return -2;
        for (uint64_t r = pile_off[i]; r < pile_off[i + 1]; r++) {
            const uint32_t *c = recs + r * 8;
            if (c[0] >= db.n_reads() || c[4] >= db.n_reads() || c[5] > c[6] || c[6] >= db.length(c[4]) || c[2] > c[3] ||
                c[3] >= db.length(c[0])) {
                fprintf(stderr, "[ndgpu] ndgpu_correct_piles: record %llu of pile %d names read %u / %u or a window outside them "
                                "(DB holds %u reads)\n", (unsigned long long)(r - pile_off[i]), i, c[0], c[4], db.n_reads());
                return -2;
            }
        }
    }
    return 0;
}

uint64_t ns_since(std::chrono::steady_clock::time_point t0) {
    return (uint64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(std::chrono::steady_clock::now() - t0).count();
}

// What the driver threads of one ndgpu_correct_piles_stream call share: the caller's arguments, the piles in launch order, the
// sub-batches' cuts and the queue over them.
struct PilesCall {
    const ReadDb *db = nullptr;
    const uint32_t *dev_pool = nullptr, *recs = nullptr;
    const uint64_t *pile_off = nullptr;
    unsigned min_len_aln = 0, max_cov_aln = 0, min_cov = 0, max_lq_length = 0, split = 0, fast = 0;
    float ratio = 0;
    int read_type = 0;
    consensus_trimed **out = nullptr;
    ndgpu_piles_done_fn done = nullptr;
    void *user = nullptr;
    std::vector<uint32_t> order;     // the piles, longest seed first
    std::vector<size_t> sub_start;   // sub-batch j = order[sub_start[j], sub_start[j + 1])
    uint64_t call_order = 0;         // (an older call in flight goes first on every context)
    int threads_each = 1;
    std::atomic<size_t> next_sub{0};
    std::atomic<uint64_t> build_ns{0}, take_ns{0};
    std::mutex done_mu;

    PileEngine *build_engine(uint32_t pid) const {
        const uint64_t r0 = pile_off[pid], r1 = pile_off[pid + 1];
        const size_t n = (size_t)(r1 - r0);
        std::vector<unsigned> st(n), en(n), len(n);
        std::vector<int64_t> dev(n);
        unsigned max_aln = n ? recs[r0 * 8 + 3] + 1 : 0;
        for (size_t i = 0; i < n; i++) {
            const uint32_t *r = recs + (r0 + i) * 8;
            dev[i] = db->window_offset(r[4], r[5], r[6], (int)r[1]);
            len[i] = r[6] - r[5] + 1;
            st[i] = r[2];
            en[i] = r[3];
            const unsigned v = r[3] - r[2] + r[6] - r[5] + 2;
            if (v > max_aln && r[0] != r[4]) max_aln = v;
        }
        const unsigned lq = n ? std::min<unsigned>(en[0] / 2, max_lq_length) : max_lq_length;
        std::string seed;  // only the HiFi consensus compares against the seed's own bases
        if (read_type == 3 && n) seed = db->window(recs[r0 * 8 + 4], recs[r0 * 8 + 5], recs[r0 * 8 + 6], 0);
        return new PileEngine(len.data(), dev.data(), st.data(), en.data(), (unsigned)n,
                              make_params(max_aln, min_len_aln, max_cov_aln, min_cov, lq, ratio, split, fast, read_type),
                              read_type == 3 ? seed.c_str() : nullptr);
    }

    void hand_over(size_t base, size_t cnt) {  // the caller's hand-over of these piles' records, while the other contexts work on
        if (!done) return;
        std::lock_guard<std::mutex> lock(done_mu);
        done(user, &order[base], (int)cnt);
    }

    // One range of the length-sorted piles through one context; out of device memory -> the context's buffers are dropped and the
    // range is halved, down to a single pile, which is then an out-of-memory seed (len 3)
    void run_range(int ctx, size_t base, size_t cnt) {
        std::vector<PileEngine *> eng(cnt, nullptr);
        const auto t_b0 = std::chrono::steady_clock::now();
        host_each(cnt, cnt <= 1, threads_each, cnt, false, [&](size_t k) { eng[k] = build_engine(order[base + k]); });
        build_ns += ns_since(t_b0);
        bool oom = false;
        {
            HipBackend be(ctx, threads_each, dev_pool, call_order, true);
            try {
                run_engines(eng.data(), cnt, be, threads_each);
            } catch (const DeviceOom &e) {
                oom = true;
                if (getenv("NDGPU_TRACE"))
                    fprintf(stderr, "[ndgpu trace] out of device memory (%zu bytes wanted) in a sub-batch of %zu piles: %s\n", e.bytes, cnt,
                            cnt > 1 ? "halved" : "reported as an out-of-memory seed (len 3)");
                // while `be` still holds the context: with two calls in flight the other call's waiting thread takes the context the
                // moment the batch ends, and its run_main's buffers must not be the ones released here
                DeviceAligner::context(ctx).release_memory();
                DeviceAligner::forget_sizes();
            }
        }
        if (oom) {
            for (PileEngine *e : eng) delete e;
            if (cnt == 1) {
                out[order[base]] = (consensus_trimed *)make_error_seed(3);
                hand_over(base, 1);
            } else {
                run_range(ctx, base, cnt / 2);
                run_range(ctx, base + cnt / 2, cnt - cnt / 2);
            }
            return;
        }
        const auto t_t0 = std::chrono::steady_clock::now();
        for (size_t k = 0; k < cnt; k++) out[order[base + k]] = (consensus_trimed *)eng[k]->take_result();
        hand_over(base, cnt);
        // tearing down the per-pile host state (thousands of small vectors per pile, ~0.3 ms each; parallel frees
        // only fight over the allocator) is not on anybody's critical path: a reaper thread does it while the caller
        // goes on, and the next call (or the library's unload) waits for it
        {
            std::lock_guard<std::mutex> lock(g_reap_mu);
            g_reapers.emplace_back([v = std::move(eng)] {
                for (PileEngine *e : v) delete e;
            });
        }
        take_ns += ns_since(t_t0);
    }

    // A driver thread: sub-batches from the call's queue through context ctx.  (The context serves this call's sub-batches one
    // behind the other before a newer call's: the place in its line is kept between them)
    void drive(int ctx) {
        DeviceAligner &dev = DeviceAligner::context(ctx);
        dev.reserve_batches(call_order);
        struct Unreserve { DeviceAligner &d; uint64_t o; ~Unreserve() { d.unreserve_batches(o); } } unreserve{dev, call_order};
        for (size_t sb; (sb = next_sub.fetch_add(1)) + 1 < sub_start.size();) run_range(ctx, sub_start[sb], sub_start[sb + 1] - sub_start[sb]);
    }
};

void print_prof(int drivers, int threads_each) {  // NDGPU_PROF: the host driver's wall-clock accounting since the last print
    fprintf(stderr, "[ndgpu prof] drivers %d x %d threads | main %.3f s  extract %.3f s  align %.3f s (%llu jobs)  "
                    "advance %.3f s  (driver-thread wall sums)\n",
            drivers, threads_each, g_prof.main_ns * 1e-9, g_prof.extract_ns * 1e-9, g_prof.align_ns * 1e-9,
            (unsigned long long)g_prof.jobs.load(), g_prof.advance_ns * 1e-9);
    fprintf(stderr, "[ndgpu prof] run_main: prep %.3f  align(K7+K8a) %.3f  tags %.3f  msa(K9+K10) %.3f  post %.3f s\n",
            g_prof.m_prep * 1e-9, g_prof.m_aln * 1e-9, g_prof.m_tags * 1e-9, g_prof.m_msa * 1e-9,
            g_prof.m_post * 1e-9);
    fprintf(stderr, "[ndgpu prof] advance, CPU seconds by phase: after main %.3f  after extract %.3f  after LQ round 1 %.3f  after round 2 + splice %.3f\n",
            g_prof.adv_ns[0] * 1e-9, g_prof.adv_ns[1] * 1e-9, g_prof.adv_ns[2] * 1e-9, g_prof.adv_ns[3] * 1e-9);
    fprintf(stderr, "[ndgpu prof] after extract: 8-mer ranking %.3f  POA %.3f  LQ round 1 layout %.3f s (CPU seconds)\n", g_prof.rank_ns * 1e-9,
            g_prof.poa_ns * 1e-9, g_prof.lqstart_ns * 1e-9);
    g_prof.rank_ns = g_prof.poa_ns = g_prof.lqstart_ns = 0;
    fprintf(stderr, "[ndgpu prof] LQ-stage alignment batches (%llu jobs): host packing %.3f s, device round trip %.3f s, host decoding %.3f s "
                    "(wall sums over contexts)\n", (unsigned long long)g_prof.c_jobs.load(), g_prof.c_pack * 1e-9, g_prof.c_dev * 1e-9,
            g_prof.c_decode * 1e-9);
    g_prof.c_pack = g_prof.c_dev = g_prof.c_decode = g_prof.c_jobs = 0;
    {   // (device counters: since the last ndgpu_reset_stats, not since the last print)
        const RuntimeStats s = DeviceAligner::total_stats();
        fprintf(stderr, "[ndgpu prof] main walks since the last reset: %llu piles, %llu path items, walk_d2h_bytes %llu | K20: cns_d2h_bytes %llu, "
                        "%llu walks, %llu declined, %llu launches, %.3f ms\n", (unsigned long long)s.piles, (unsigned long long)s.path_items,
                (unsigned long long)s.walk_d2h_bytes, (unsigned long long)s.cns_d2h_bytes, (unsigned long long)s.cns_jobs,
                (unsigned long long)s.cns_declined, (unsigned long long)s.cns_launches, s.cns_ms);
        fprintf(stderr, "[ndgpu prof] K21 since the last reset: d2h_bytes %llu, HiFi %llu walks, %llu declined, %llu windows | -fast %llu walks, "
                        "%llu declined | %llu launches, %.3f ms\n", (unsigned long long)s.cnsw_d2h_bytes, (unsigned long long)s.cnsw_hifi_jobs,
                (unsigned long long)s.cnsw_hifi_declined, (unsigned long long)s.cnsw_hifi_regions, (unsigned long long)s.cnsw_fast_jobs,
                (unsigned long long)s.cnsw_fast_declined, (unsigned long long)s.cnsw_launches, s.cnsw_ms);
        uint64_t declined = 0;
        for (int k = 0; k < 5; k++) declined += s.phase_declined[k];
        fprintf(stderr, "[ndgpu prof] K22 since the last reset: %llu piles, %llu regions (%llu seed, %llu ranked, %llu dropped), %llu declined | "
                        "%llu launches, %.3f ms | d2h: records %llu bytes, strings %llu bytes\n", (unsigned long long)s.phase_piles,
                (unsigned long long)s.phase_regions, (unsigned long long)s.phase_kind[2], (unsigned long long)s.phase_kind[3],
                (unsigned long long)s.phase_kind[1], (unsigned long long)declined, (unsigned long long)s.phase_launches, s.phase_ms,
                (unsigned long long)s.phase_d2h_records, (unsigned long long)s.phase_d2h_strings);
        fprintf(stderr, "[ndgpu prof] K24 since the last reset: %llu jobs, %llu declined, %llu trimmed | %llu launches, %.3f ms | h2d %llu bytes, "
                        "d2h %llu bytes\n", (unsigned long long)s.splice_jobs, (unsigned long long)s.splice_declined,
                (unsigned long long)s.splice_trimmed, (unsigned long long)s.splice_launches, s.splice_ms,
                (unsigned long long)s.splice_h2d_bytes, (unsigned long long)s.splice_d2h_bytes);
    }
    for (auto &a : g_prof.adv_ns) a = 0;
    g_prof.main_ns = g_prof.extract_ns = g_prof.align_ns = g_prof.advance_ns = g_prof.jobs = 0;
    g_prof.m_prep = g_prof.m_aln = g_prof.m_tags = g_prof.m_msa = g_prof.m_post = 0;
}

}  // namespace

extern "C" {

consensus_trimed *nextCorrect(char **seqs, unsigned int *aln_start, unsigned int *aln_end, unsigned int seq_count,
                              unsigned int max_mem_len, unsigned int min_len_aln, unsigned int max_cov_aln,
                              unsigned int min_cov, unsigned int lqseq_max_length, float min_error_corrected_ratio,
                              unsigned int split, unsigned int fast, int read_type) {
    PileEngine eng(seqs, aln_start, aln_end, seq_count,
                   make_params(max_mem_len, min_len_aln, max_cov_aln, min_cov, lqseq_max_length,
                               min_error_corrected_ratio, split, fast, read_type));
    PileEngine *ep = &eng;
    try {
        HipBackend be;
        run_engines(&ep, 1, be, 1);
    } catch (const DeviceOom &) {  // lib/nextcorrect.c:2254-2261: a seed whose working memory cannot be had is reported, not fatal
        DeviceAligner::context(0).release_memory();
        DeviceAligner::forget_sizes();
        return (consensus_trimed *)make_error_seed(3);
    }
    return (consensus_trimed *)eng.take_result();
}

void free_consensus_trimed(consensus_trimed *c) {
    if (!c) return;
    free(c->seq);
    free(c);
}

// lib/nextcorrect.py:236-260 over the records of one hand-over: headers and index lines are formatted into two small buffers, the
// bases go to the file from where the library holds them (writev: no copy of the 70 MB a config-2 step prints)
int ndgpu_write_records(consensus_trimed **recs, const uint32_t *ids, int n, const uint32_t *names, uint32_t min_len_seed,
                        double min_ratio, int fd_out, int fd_idx, uint64_t *pos, uint32_t *lens, float *identities) {
    std::vector<char> heads;
    std::string idx;
    struct Piece { size_t head_at, head_len; const char *seq; size_t len; };
    std::vector<Piece> pieces;
    heads.reserve((size_t)n * 40);
    uint64_t at = *pos;
    char line[96];
    for (int k = 0; k < n; k++) {
        const uint32_t i = ids[k];
        consensus_trimed *c = recs[i];
        if (!c) continue;
        const uint32_t ln = c->len;
        const float ide = c->identity;
        if (lens) lens[i] = ln;
        if (identities) identities[i] = ide;
        if (ln >= min_len_seed && ln > 4 && (double)ide >= min_ratio) {
            const int hl = snprintf(line, sizeof(line), ">%u %u %f\n", names[i], ln, (double)ide);
            pieces.push_back(Piece{heads.size(), (size_t)hl, c->seq, (size_t)ln});
            heads.insert(heads.end(), line, line + hl);
            at += (uint64_t)hl + ln + 1;
            if (fd_idx >= 0) {
                const int il = snprintf(line, sizeof(line), "%u\t%llu\t%u\n", names[i], (unsigned long long)(at - ln - 1), ln);
                idx.append(line, (size_t)il);
            }
        } else if (ln != 3 && fd_idx >= 0) {
            const int il = snprintf(line, sizeof(line), "%u\t0\t0\n", names[i]);
            idx.append(line, (size_t)il);
        }
    }
    auto write_all = [](int fd, struct iovec *iov, int cnt) {
        while (cnt > 0) {
            ssize_t w = writev(fd, iov, cnt > 1024 ? 1024 : cnt);
            if (w < 0 && errno == EINTR) continue;   // (a signal, not a failure)
            if (w < 0) return false;
            while (cnt > 0 && (size_t)w >= iov->iov_len) w -= (ssize_t)iov->iov_len, ++iov, --cnt;
            if (cnt > 0 && w > 0) iov->iov_base = (char *)iov->iov_base + w, iov->iov_len -= (size_t)w;
        }
        return true;
    };
    bool ok = true;
    static const char nl = '\n';
    std::vector<struct iovec> iov;
    iov.reserve(pieces.size() * 3);
    for (const Piece &p : pieces) {
        iov.push_back({heads.data() + p.head_at, p.head_len});
        iov.push_back({(void *)p.seq, p.len});
        iov.push_back({(void *)&nl, 1});
    }
    const off_t idx0 = fd_idx >= 0 ? lseek(fd_idx, 0, SEEK_CUR) : (off_t)-1;   // (where the index stood before this hand-over)
    if (!iov.empty()) ok = write_all(fd_out, iov.data(), (int)iov.size());
    if (ok && fd_idx >= 0 && !idx.empty()) {
        struct iovec one{(void *)idx.data(), idx.size()};
        ok = write_all(fd_idx, &one, 1);
    }
    for (int k = 0; k < n; k++) {   // (after the write: the bases were the library's until here)
        free_consensus_trimed(recs[ids[k]]);
        recs[ids[k]] = nullptr;
    }
    if (ok) *pos = at;
    else {
        // part of the hand-over may be on disk and its index lines not: cut both files back to where they stood before this call, so
        // that what a resumed run reads (lib/nextcorrect.py:205-226: the .idx decides where the .fasta is cut) belongs together
        if (ftruncate(fd_out, (off_t)*pos) == 0) (void)lseek(fd_out, (off_t)*pos, SEEK_SET);
        if (idx0 >= 0 && ftruncate(fd_idx, idx0) == 0) (void)lseek(fd_idx, idx0, SEEK_SET);
    }
    return ok ? 0 : -1;
}

int ndgpu_correct_batch(int n_piles, char ***seqs, unsigned int **aln_start, unsigned int **aln_end,
                        const unsigned int *seq_count, const unsigned int *max_mem_len,
                        const unsigned int *lqseq_max_length, unsigned int min_len_aln, unsigned int max_cov_aln,
                        unsigned int min_cov, float min_error_corrected_ratio, unsigned int split, unsigned int fast,
                        int read_type, int host_threads, consensus_trimed **out) {
    if (n_piles <= 0) return 0;
    // (what the process can have, not what the machine has: a cgroup quota of 16 CPUs on a 256-thread host; asking for more only
    // gets the whole process throttled)
    if (host_threads <= 0 || (host_threads > effective_cpus() && !getenv("NDGPU_NO_CPU_CAP"))) host_threads = effective_cpus();
    std::vector<PileEngine *> eng((size_t)n_piles, nullptr);
    host_each((size_t)n_piles, host_threads <= 1 || n_piles <= 1, host_threads, (size_t)n_piles, false, [&](size_t i) {
        eng[i] = new PileEngine(seqs[i], aln_start[i], aln_end[i], seq_count[i],
                                make_params(max_mem_len[i], min_len_aln, max_cov_aln, min_cov, lqseq_max_length[i],
                                            min_error_corrected_ratio, split, fast, read_type));
    });
    // (out of device memory: the batch is halved until it fits; a single pile that does not fit is an out-of-memory seed)
    std::vector<std::pair<size_t, size_t>> todo{{0, (size_t)n_piles}};
    while (!todo.empty()) {
        const auto [a, b] = todo.back();
        todo.pop_back();
        try {
            HipBackend be(0, host_threads);
            run_engines(eng.data() + a, b - a, be, host_threads);
            for (size_t i = a; i < b; i++) out[i] = (consensus_trimed *)eng[i]->take_result();
        } catch (const DeviceOom &) {
            DeviceAligner::context(0).release_memory();
            DeviceAligner::forget_sizes();
            for (size_t i = a; i < b; i++) {  // engines restart from scratch
                delete eng[i];
                eng[i] = new PileEngine(seqs[i], aln_start[i], aln_end[i], seq_count[i],
                                        make_params(max_mem_len[i], min_len_aln, max_cov_aln, min_cov, lqseq_max_length[i],
                                                    min_error_corrected_ratio, split, fast, read_type));
            }
            if (b - a == 1) out[a] = (consensus_trimed *)make_error_seed(3);
            else {
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    for (size_t i = 0; i < (size_t)n_piles; i++) delete eng[i];
    return 0;
}

struct ndgpu_db {
    ReadDb *db;
    uint32_t *dev_pool;  // this handle's copy in HBM (forward + reverse complement), handed to every batch that names it
};

ndgpu_db *ndgpu_db_create(uint32_t n_reads, const uint32_t *words, const uint64_t *word_off, const uint32_t *len) {
    ndgpu_db *h = new ndgpu_db;
    h->db = new ReadDb(n_reads, words, word_off, len);
    h->dev_pool = DeviceAligner::upload_db(h->db->pool().data(), h->db->pool().size(), DeviceAligner::instance().device());
    if (!h->dev_pool) {
        fprintf(stderr, "[ndgpu] ndgpu_db_create: out of device memory for a read DB of %llu bases\n",
                (unsigned long long)h->db->total_bases());
        delete h->db;
        delete h;
        return nullptr;
    }
    return h;
}

// init_ovls()'s view of the read DB (lib/ovlseq.c:50-138, lib/index.c:7-36): `idx_fofn` lists one `.idx` per line, the
// `.2bit` of `/dir/.NAME.idx` is `/dir/NAME.2bit` (lib/ovlseq.c:24-37); a `.2bit` holds {0, 254}, then per read u32 id,
// u32 length, ceil(length / 16) words (lib/bseq.c:93-139).  Read ids index the DB.  NULL on any I/O or format error.
ndgpu_db *ndgpu_db_open(const char *idx_fofn) {
    FILE *f = fopen(idx_fofn, "r");
    if (!f) {
        fprintf(stderr, "[ndgpu] ndgpu_db_open: cannot open %s\n", idx_fofn);
        return nullptr;
    }
    std::vector<std::string> idx_files;
    char line[4096];
    while (fgets(line, sizeof(line), f)) {
        std::string s(line);
        while (!s.empty() && (s.back() == '\n' || s.back() == '\r' || s.back() == ' ')) s.pop_back();
        if (!s.empty() && s[0] != '#') idx_files.push_back(s);
    }
    fclose(f);
    std::vector<uint32_t> words, lens;
    std::vector<uint64_t> word_off;
    // ids index the DB: bound them by the number of lines of the .idx files (one per read, lib/index.c:7-36) -- a corrupt id
    // must not size the tables
    size_t max_reads = 0;
    for (const std::string &idx : idx_files) {
        FILE *t = fopen(idx.c_str(), "r");
        if (!t) {
            fprintf(stderr, "[ndgpu] ndgpu_db_open: cannot open %s\n", idx.c_str());
            return nullptr;
        }
        char buf[65536];
        size_t got;
        while ((got = fread(buf, 1, sizeof(buf), t)) > 0)
            for (size_t i = 0; i < got; i++) max_reads += buf[i] == '\n';
        fclose(t);
        max_reads++;  // a last line without a newline
    }
    for (const std::string &idx : idx_files) {
        const size_t slash = idx.find_last_of('/');
        const std::string dir = slash == std::string::npos ? "" : idx.substr(0, slash + 1);
        std::string name = slash == std::string::npos ? idx : idx.substr(slash + 1);
        if (name.size() < 6 || name[0] != '.' || name.substr(name.size() - 4) != ".idx") {
            fprintf(stderr, "[ndgpu] ndgpu_db_open: %s is not a .NAME.idx path\n", idx.c_str());
            return nullptr;
        }
        const std::string path = dir + name.substr(1, name.size() - 5) + ".2bit";
        FILE *b = fopen(path.c_str(), "rb");
        if (!b) {
            fprintf(stderr, "[ndgpu] ndgpu_db_open: cannot open %s\n", path.c_str());
            return nullptr;
        }
        fseek(b, 0, SEEK_END);
        const long sz = ftell(b);
        fseek(b, 2, SEEK_SET);
        const size_t nw = sz > 2 ? (size_t)(sz - 2) / 4 : 0;
        const size_t base = words.size();
        words.resize(base + nw);
        if (nw && fread(words.data() + base, 4, nw, b) != nw) {
            fclose(b);
            fprintf(stderr, "[ndgpu] ndgpu_db_open: short read on %s\n", path.c_str());
            return nullptr;
        }
        fclose(b);
        for (size_t p = base; p + 2 <= base + nw;) {
            const uint32_t id = words[p], ln = words[p + 1];
            if (p + 2 + (((size_t)ln + 15) >> 4) > base + nw || (size_t)id >= max_reads) {  // truncated / corrupt file
                fprintf(stderr, "[ndgpu] ndgpu_db_open: %s: record at word %zu (id %u, %u bases) %s\n", path.c_str(), p - base, id, ln,
                        (size_t)id >= max_reads ? "names a read the .idx files do not list" : "runs past the end of the file");
                return nullptr;
            }
            if (id >= lens.size()) {
                lens.resize((size_t)id + 1, 0);
                word_off.resize((size_t)id + 1, 0);
            }
            lens[id] = ln;
            word_off[id] = p + 2;
            p += 2 + (((size_t)ln + 15) >> 4);
        }
    }
    return ndgpu_db_create((uint32_t)lens.size(), words.data(), word_off.data(), lens.data());
}

void ndgpu_db_destroy(ndgpu_db *h) {
    if (!h) return;
    join_reapers();
    DeviceAligner::free_db(h->dev_pool);
    delete h->db;
    delete h;
}


int ndgpu_correct_piles(ndgpu_db *h, int n_piles, const uint32_t *recs, const uint64_t *pile_off,
                        unsigned int min_len_aln, unsigned int max_cov_aln, unsigned int min_cov,
                        unsigned int max_lq_length, float min_error_corrected_ratio, unsigned int split,
                        unsigned int fast, int read_type, int host_threads, consensus_trimed **out) {
    return ndgpu_correct_piles_stream(h, n_piles, recs, pile_off, min_len_aln, max_cov_aln, min_cov, max_lq_length, min_error_corrected_ratio,
                                      split, fast, read_type, host_threads, out, nullptr, nullptr);
}

int ndgpu_correct_piles_stream(ndgpu_db *h, int n_piles, const uint32_t *recs, const uint64_t *pile_off,
                               unsigned int min_len_aln, unsigned int max_cov_aln, unsigned int min_cov,
                               unsigned int max_lq_length, float min_error_corrected_ratio, unsigned int split,
                               unsigned int fast, int read_type, int host_threads, consensus_trimed **out,
                               ndgpu_piles_done_fn done, void *user) {
    if (n_piles <= 0) return 0;
    if (!h || !h->db || !h->dev_pool) return -1;
    // (what the process can have, not what the machine has: a cgroup quota of 16 CPUs on a 256-thread host; asking for more only
    // gets the whole process throttled)
    if (host_threads <= 0 || (host_threads > effective_cpus() && !getenv("NDGPU_NO_CPU_CAP"))) host_threads = effective_cpus();
    if (const int rc = validate_records(*h->db, n_piles, recs, pile_off)) return rc;
    join_reapers();  // the previous call's teardown
    PilesCall call;
    call.db = h->db, call.dev_pool = h->dev_pool, call.recs = recs, call.pile_off = pile_off;
    call.min_len_aln = min_len_aln, call.max_cov_aln = max_cov_aln, call.min_cov = min_cov, call.max_lq_length = max_lq_length;
    call.ratio = min_error_corrected_ratio, call.split = split, call.fast = fast, call.read_type = read_type;
    call.out = out, call.done = done, call.user = user;
    call.call_order = DeviceAligner::next_order();
    const auto t_call0 = std::chrono::steady_clock::now();
    // piles per sub-batch at most (the cost target normally cuts earlier)
    size_t sub = 384;
    if (const char *e = getenv("NDGPU_SUBBATCH")) sub = (size_t)std::max(1, atoi(e));
    // longest seeds first: the scoring DP is a sequential chain per seed, so similar lengths
    // share a launch and the long chains start early
    std::vector<uint32_t> &order = call.order;
    order.resize((size_t)n_piles);
    for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
        return recs[pile_off[a] * 8 + 3] > recs[pile_off[b] * 8 + 3];
    });
    int drivers = 8;
    // (a context is a host thread that launches and waits: with fewer CPUs than contexts -- a rank of 8 on a node whose container has 16
    // -- the contexts only take the CPUs from one another's host phases)
    drivers = std::min(drivers, std::max(2, host_threads));
    if (const char *e = getenv("NDGPU_CONTEXTS")) drivers = std::max(1, std::min(atoi(e), (int)DeviceAligner::kMaxContexts));
    // sub-batches (nd_subplan.h): at most `sub` piles and at most `tag_budget` estimated alignment columns each
    uint64_t tag_budget = 900000000ull;
    DeviceAligner::plan_memory(drivers, &tag_budget);  // what the device has free now decides it
    if (const char *e = getenv("NDGPU_SUBBATCH_TAGS")) tag_budget = std::max<uint64_t>(1000000ull, strtoull(e, nullptr, 10));
    std::vector<uint64_t> est((size_t)n_piles);  // cost of a pile = its estimated alignment columns
    for (size_t k = 0; k < (size_t)n_piles; k++) {
        const uint32_t pid = order[k];
        uint64_t e = 0;
        for (uint64_t r = pile_off[pid]; r < pile_off[pid + 1]; r++) e += (uint64_t)(recs[r * 8 + 3] - recs[r * 8 + 2] + 1);
        est[k] = e + e / 6;
    }
    int per_ctx = n_piles >= 1024 ? 2 : 1;  // (a small call is a matter of latency: see plan_sub_batches)
    if (const char *e = getenv("NDGPU_SUBBATCHES_PER_CONTEXT")) per_ctx = std::max(1, atoi(e));
    call.sub_start = plan_sub_batches(est, drivers, round_weights(per_ctx, getenv("NDGPU_TAPER")), sub, tag_budget);
    const size_t n_sub = call.sub_start.size() - 1;
    drivers = (int)std::min<size_t>((size_t)drivers, n_sub);
    int threads_each = std::max(1, host_threads / drivers);  // (measured: more threads per context is slower)
    if (const char *e = getenv("NDGPU_THREADS_PER_CONTEXT")) threads_each = std::max(1, atoi(e));
    call.threads_each = threads_each;
    CoreGovernor::set_total(getenv("NDGPU_NO_BORROW") ? 0 : host_threads);
    std::vector<std::thread> th;
    for (int c = 1; c < drivers; c++) th.emplace_back([&call, c] { call.drive(c); });
    call.drive(0);
    for (auto &t : th) t.join();
    DeviceAligner::level_buffers(drivers);  // (nothing in flight now) no context will have to grow a buffer in the middle of the next call
    if (getenv("NDGPU_TRACE"))
        fprintf(stderr, "[ndgpu trace] correct_piles %d piles in %zu sub-batches: %.1f ms wall | engine build %.1f ms, result take %.1f ms (summed over contexts)\n",
                n_piles, n_sub, std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_call0).count() * 1e-3,
                call.build_ns.load() * 1e-6, call.take_ns.load() * 1e-6);
    if (getenv("NDGPU_PROF")) print_prof(drivers, threads_each);
    return 0;
}

void align(char *query_seq, int q_len, char *target_seq, int t_len, alignment *align_rtn, int *, uint8_t **) {
    run_single_alignment(query_seq, q_len, target_seq, t_len, align_rtn, 0);
}

void align_hq(char *query_seq, int q_len, char *target_seq, int t_len, alignment *align_rtn, int *, uint8_t **) {
    run_single_alignment(query_seq, q_len, target_seq, t_len, align_rtn, 1);
}

// replaces lib/align.c:580-679 (`align_nd`: global alignment, match 2 / mismatch -4 / gap open -4 / gap extend -2, two
// traceback bits per cell packed four to a byte).  Exported by the reference's nextcorrect.so but called from nowhere
// (its one call site, lib/ctg_cns.c:1357, is commented out), so it stays a host routine.  The definition names its
// parameters (s2, s2_l, s1, s1_l): the FIRST sequence indexes the columns; rows are written to t_aln_str.
void align_nd(const char *s2, const uint32_t s2_l, const char *s1, const uint32_t s1_l, alignment *aln) {
    static const uint8_t MMH[4] = {64, 16, 4, 1}, INS[4] = {128, 32, 8, 2}, DEL[4] = {192, 48, 12, 3};
    const int mas = 2, mis = -4, gos = -4, ges = -2;
    const size_t row = ((size_t)s2_l >> 2) + 1;
    std::vector<uint8_t> dm(row * ((size_t)s1_l + 1), 0);
    auto d = [&](uint32_t i) { return dm.data() + row * (size_t)i; };
    std::vector<int32_t> sc((size_t)s2_l + 1, 0);
    int32_t cs = 0;
    d(0)[0] |= MMH[0];
    for (uint32_t j = 1; j <= s2_l; j++) {
        sc[j] = sc[j - 1] + ((d(0)[(j - 1) >> 2] & DEL[(j - 1) & 3]) == DEL[(j - 1) & 3] ? ges : gos);
        d(0)[j >> 2] |= DEL[j & 3];
    }
    for (uint32_t i = 1; i <= s1_l; i++) {
        uint8_t *di = d(i);
        const uint8_t *dp = d(i - 1);
        for (uint32_t j = 0; j <= s2_l; j++) {
            if (j == 0) {
                cs = sc[0] + ((dp[0] & DEL[0]) == INS[0] ? ges : gos);
                di[0] = INS[0];
            } else {
                const uint32_t k = j & 3;
                const int32_t ms = sc[j - 1] + (s1[i - 1] == s2[j - 1] ? mas : mis);
                const int32_t is = sc[j] + ((dp[j >> 2] & DEL[k]) == INS[k] ? ges : gos);
                const int32_t ds = cs + ((di[(j - 1) >> 2] & DEL[(j - 1) & 3]) == DEL[(j - 1) & 3] ? ges : gos);
                sc[j - 1] = cs;
                uint8_t mv;
                if (ms > is) {
                    if (ms > ds) cs = ms, mv = MMH[k];
                    else cs = ds, mv = DEL[k];
                } else {
                    if (is > ds) cs = is, mv = INS[k];
                    else cs = ds, mv = DEL[k];
                }
                di[j >> 2] |= mv;
                if (j == s2_l) sc[j] = cs;
            }
        }
    }
    uint32_t a = s1_l, b = s2_l, n = 0;
    while (a != 0 || b != 0) {
        const uint32_t k = b & 3;
        const uint8_t mv = d(a)[b >> 2] & DEL[k];
        if (mv == MMH[k]) {
            aln->t_aln_str[n] = s1[--a];
            aln->q_aln_str[n] = s2[--b];
        } else if (mv == DEL[k]) {
            aln->q_aln_str[n] = s2[--b];
            aln->t_aln_str[n] = '-';
        } else {
            aln->t_aln_str[n] = s1[--a];
            aln->q_aln_str[n] = '-';
        }
        n++;
    }
    aln->aln_len = n;
    aln->t_aln_str[n] = aln->q_aln_str[n] = '\0';
    reverse_str(aln->t_aln_str, (int)n);
    reverse_str(aln->q_aln_str, (int)n);
}

// The device owns the DP state; these exist so that code written against
// lib/align.h links unchanged.  V gets the reference's size, D a 1-slot table.
void malloc_vd(int **V, uint8_t ***D, uint64_t max_mem_d) {
    *V = (int *)malloc((size_t)(max_mem_d ? max_mem_d : 1) * 2 * sizeof(int));
    *D = (uint8_t **)calloc(1, sizeof(uint8_t *));
}
void clean_V(int *V, int max_mem_d) {
    if (V && max_mem_d > 0) memset(V, 0, (size_t)max_mem_d * 2 * sizeof(int));
}
void destory_vd(int *V, uint8_t **D) {
    free(V);
    free(D);
}

void reverse_str(char *str, int len) {
    for (int a = 0, b = len - 1; a < b; a++, b--) std::swap(str[a], str[b]);
}

void revcomp_bseq(char *str, int len) {
    // complement table semantics of lib/align.c:3-20 for the IUPAC letters it maps
    static const char *from = "ACGTUMRWSYKVHDBNacgtumrwsykvhdbn";
    static const char *to = "TGCAAKYWSRMBDHVNtgcaakywsrmbdhvn";
    static unsigned char lut[256];
    static bool init = false;
    if (!init) {
        for (int i = 0; i < 256; i++) lut[i] = (unsigned char)i;
        for (int i = 0; from[i]; i++) lut[(unsigned char)from[i]] = (unsigned char)to[i];
        init = true;
    }
    int a = 0, b = len - 1;
    while (a < b) {
        const unsigned char x = lut[(unsigned char)str[a]], y = lut[(unsigned char)str[b]];
        str[a++] = (char)y;
        str[b--] = (char)x;
    }
    if (a == b) str[a] = (char)lut[(unsigned char)str[a]];
}

void str_tolower(char *p) {
    for (; *p; ++p) *p |= 0x20;
}
void str_toupper(char *p) {
    for (; *p; ++p) *p &= (char)0xdf;
}

char *poa_to_consensus(const void *seqs, const int seq_count) {
    // struct seq_ { uint16_t order, kscore, len; char seq[10000]; }  (lib/nextcorrect.h:63-68)
    const size_t stride = 3 * sizeof(uint16_t) + 10000;
    std::vector<std::string> in;
    for (int i = 0; i < seq_count; i++) {
        const unsigned char *rec = (const unsigned char *)seqs + (size_t)i * stride;
        uint16_t len;
        memcpy(&len, rec + 4, sizeof(len));
        in.emplace_back((const char *)rec + 6, (size_t)len);
    }
    std::string r = poa_consensus(in);
    char *out = (char *)malloc(r.size() + 1);
    memcpy(out, r.c_str(), r.size() + 1);
    return out;
}

// poa_to_consensus for a batch of problems: the alignments on the device in lockstep rounds (DeviceAligner::run_poa); a problem
// the device declines is computed by the host path here, in the same call
int ndgpu_poa_batch(const ndgpu_poa_job *jobs, int n, char **out) { return ndgpu_poa_batch_flags(jobs, n, 0, out); }

// flags: bit 0 the host routine for every job; bit 1 resident graphs (K19), bit 2 K13's rounds, whatever NDGPU_POA_RESIDENT says
int ndgpu_poa_batch_flags(const ndgpu_poa_job *jobs, int n, int flags, char **out) {
    if ((flags & ~7) != 0 || (flags & 6) == 6) return -2;
    if (n <= 0) return 0;
    const bool host_only = (flags & 1) != 0;
    const int form = flags & 2 ? 1 : flags & 4 ? 2 : 0;
    int n_dev = 0;
    if (!host_only && (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)) {
        fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_poa_batch runs its alignments on the device\n");
        return -1;
    }
    std::vector<PoaReq> reqs((size_t)n);
    std::vector<PoaReq *> ptr((size_t)n);
    for (int i = 0; i < n; i++) {
        out[i] = nullptr;
        if (jobs[i].seq_count < 0 || jobs[i].seq_count > kPoaMaxSeqs) return -2;
        for (int k = 0; k < jobs[i].seq_count; k++) reqs[i].seqs.emplace_back(jobs[i].seqs[k], (size_t)jobs[i].len[k]);
        ptr[i] = &reqs[i];
    }
    const int threads = effective_cpus();
    // (out of device memory: the range is halved until it fits; a single problem that does not fit goes the host way)
    std::vector<std::pair<size_t, size_t>> todo{{0, (size_t)n}};
    if (host_only) todo.clear();
    while (!todo.empty()) {
        const auto [a, b] = todo.back();
        todo.pop_back();
        try {
            HipBackend be(0, threads);
            if (form) be.run_poa_form(ptr.data() + a, b - a, form);
            else (void)be.run_poa(ptr.data() + a, b - a);
        } catch (const DeviceOom &) {
            DeviceAligner::context(0).release_memory();
            DeviceAligner::forget_sizes();
            if (b - a > 1) {
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    int rc = 0;
    host_each((size_t)n, threads <= 1 || n <= 1, threads, (size_t)n, false, [&](size_t i) {
        PoaReq &rq = reqs[i];
        if (!rq.done && !rq.failed) {
            rq.out = poa_consensus(rq.seqs);
            rq.done = true;
        }
    });
    for (int i = 0; i < n; i++) {
        if (reqs[i].failed) {
            rc = -3;
            continue;
        }
        out[i] = (char *)malloc(reqs[i].out.size() + 1);
        memcpy(out[i], reqs[i].out.c_str(), reqs[i].out.size() + 1);
    }
    if (rc)
        for (int i = 0; i < n; i++) free(out[i]), out[i] = nullptr;
    return rc;
}

// The 8-mer ranking of a batch of candidate sets: K14 on the device (DeviceAligner::run_rank), or -- flags bit 0 -- the engine's own
// host routine (lq_rank_host)
int ndgpu_lq_rank_batch(const ndgpu_rank_job *jobs, int n, int flags, ndgpu_rank_result *res) {
    if (n <= 0) return 0;
    for (int i = 0; i < n; i++)
        if (jobs[i].seq_count < 1 || jobs[i].seq_count > kLqRankMax) return -2;
    std::vector<RankReq> reqs((size_t)n);
    for (int i = 0; i < n; i++) reqs[i].seqs = jobs[i].seqs, reqs[i].len = jobs[i].len, reqs[i].n = jobs[i].seq_count;
    if (flags & 1) {
        host_each((size_t)n, effective_cpus() <= 1 || n <= 1, effective_cpus(), (size_t)n, false, [&](size_t i) {
            RankReq &rq = reqs[i];
            lq_rank_host(rq.seqs, rq.len, rq.n, rq.order, rq.kscore, &rq.tail);
        });
    } else {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
            fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_lq_rank_batch ranks on the device unless flags bit 0 is set\n");
            return -1;
        }
        // (out of device memory: the range is halved until it fits)
        std::vector<std::pair<size_t, size_t>> todo{{0, (size_t)n}};
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            try {
                HipBackend be(0, 1);
                be.run_rank(reqs.data() + a, b - a);
            } catch (const DeviceOom &) {
                DeviceAligner::context(0).release_memory();
                DeviceAligner::forget_sizes();
                if (b - a <= 1) return -3;
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    for (int i = 0; i < n; i++) {
        memset(&res[i], 0, sizeof(res[i]));
        memcpy(res[i].order, reqs[i].order, (size_t)reqs[i].n);
        memcpy(res[i].kscore, reqs[i].kscore, (size_t)reqs[i].n * sizeof(uint16_t));
        res[i].tail = reqs[i].tail;
    }
    return 0;
}

// The phasing and ranking of the candidates of a batch of HiFi piles: K22 on the device (DeviceAligner::run_phase), or -- flags bit 0 --
// the engine's own host rule (hifi_phase_host of nd_phase.h); a pile the kernel declines takes the host rule too.
int ndgpu_hifi_phase_batch(const ndgpu_phase_job *jobs, int n, int flags, ndgpu_phase_region *regions_out, ndgpu_phase_pile *piles_out) {
    static_assert(sizeof(ndgpu_phase_region) == sizeof(PhaseRecord), "the records are copied as they stand");
    if (n == 0) return 0;
    if (n < 0 || !jobs || !piles_out) return -2;
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        const ndgpu_phase_job &j = jobs[i];
        if (j.n_regions && !j.regions) return -2;
        for (uint32_t r = 0; r < j.n_regions; r++) {
            const ndgpu_phase_region_in &g = j.regions[r];
            if (g.n_cand < 0 || g.n_cand > kPhaseCanMax) return -2;
            if (g.n_cand && (!g.seqs || !g.len || !g.src)) return -2;
            for (int c = 0; c < g.n_cand; c++)
                if ((g.len[c] && !g.seqs[c]) || g.src[c] >= j.n_aligned) return -2;
        }
        total += j.n_regions;
    }
    if (total && !regions_out) return -2;
    std::vector<PhaseRegionIn> in(total);
    std::vector<PhaseRecord> recs(total);
    std::vector<PhaseReq> reqs((size_t)n);
    for (size_t i = 0, at = 0; i < (size_t)n; i++) {
        const ndgpu_phase_job &j = jobs[i];
        for (uint32_t r = 0; r < j.n_regions; r++) {
            const ndgpu_phase_region_in &g = j.regions[r];
            in[at + r] = PhaseRegionIn{g.start, g.end, g.n_cand, g.seqs, g.len, g.src};
        }
        reqs[i].n_aligned = j.n_aligned, reqs[i].regions = in.data() + at, reqs[i].n_regions = j.n_regions, reqs[i].out = recs.data() + at;
        at += j.n_regions;
    }
    if (!(flags & 1)) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
            fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_hifi_phase_batch runs on the device unless flags bit 0 is set\n");
            return -1;
        }
        // (out of device memory: the range is halved until it fits)
        std::vector<std::pair<size_t, size_t>> todo{{0, (size_t)n}};
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            try {
                HipBackend be(0, 1);
                be.run_phase(reqs.data() + a, b - a);
            } catch (const DeviceOom &) {
                DeviceAligner::context(0).release_memory();
                DeviceAligner::forget_sizes();
                if (b - a <= 1) continue;   // (a single pile that does not fit: declined, the host rule takes it)
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    host_each((size_t)n, effective_cpus() <= 1 || n <= 1, effective_cpus(), (size_t)n, false, [&](size_t i) {
        PhaseReq &rq = reqs[i];
        piles_out[i].declined = !(flags & 1) && !rq.done ? 1 : 0;
        if (!rq.done) hifi_phase_host(rq.n_aligned, rq.regions, rq.n_regions, rq.out, rq.pile);
        piles_out[i].has_heter = rq.pile.has_heter, piles_out[i].pass2 = rq.pile.pass2, piles_out[i].pad_ = 0;
    });
    if (total) memcpy(regions_out, recs.data(), total * sizeof(PhaseRecord));
    return 0;
}

// The consensus words and low-quality windows of a batch of walks: K20 on the device (DeviceAligner::run_cns), or -- flags bit 0 -- the
// engine's own host routine (cns_windows_host); a walk the kernel declines takes the host routine too.  The verdict is cns_verdict.
int ndgpu_cns_windows_batch(const ndgpu_cns_job *jobs, int n, int flags, ndgpu_cns_result *res, uint32_t **bases, uint32_t **regions) {
    if (n == 0) return 0;
    if (n < 0 || !jobs || !res || !bases || !regions) return -2;
    size_t total = 0;
    for (int i = 0; i < n; i++) {
        if (jobs[i].n && !jobs[i].steps) return -2;
        for (uint32_t k = 0; k < jobs[i].n; k++) {
            const ndgpu_walk_step &s = jobs[i].steps[k];
            if (s.base == 4) continue;
            if (s.cov == 0 || s.base > 5 || s.t_pos < 0 || s.t_pos > (1 << 21) - 2) return -2;   // (t_pos + 1 has 21 bits in the tag)
        }
        total += jobs[i].n;
    }
    std::vector<PathStep> steps(total);
    std::vector<CnsReq> reqs((size_t)n);
    for (size_t i = 0, at = 0; i < (size_t)n; i++) {
        const ndgpu_cns_job &j = jobs[i];
        for (uint32_t k = 0; k < j.n; k++) {
            PathStep &d = steps[at + k];
            d.t_pos = j.steps[k].t_pos, d.delta = 0, d.base = j.steps[k].base, d.link = j.steps[k].link, d.cov = j.steps[k].cov;
        }
        reqs[i].steps = steps.data() + at, reqs[i].n = j.n, reqs[i].min_cov = j.min_cov, reqs[i].lq_max_len = j.lq_max_len;
        at += j.n;
    }
    if (!(flags & 1)) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
            fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_cns_windows_batch runs on the device unless flags bit 0 is set\n");
            return -1;
        }
        // (out of device memory: the range is halved until it fits)
        std::vector<std::pair<size_t, size_t>> todo{{0, (size_t)n}};
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            try {
                HipBackend be(0, 1);
                be.run_cns(reqs.data() + a, b - a);
            } catch (const DeviceOom &) {
                DeviceAligner::context(0).release_memory();
                DeviceAligner::forget_sizes();
                if (b - a <= 1) return -3;
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    host_each((size_t)n, effective_cpus() <= 1 || n <= 1, effective_cpus(), (size_t)n, false, [&](size_t i) {
        CnsReq &rq = reqs[i];
        if (rq.done) return;
        std::vector<CnsWindow> wins;
        CnsCounts c;
        cns_windows_host(rq.steps, rq.n, rq.min_cov, rq.lq_max_len, rq.words, wins, c);
        rq.wins.clear();
        for (const CnsWindow &w : wins) rq.wins.push_back(w.start), rq.wins.push_back(w.end);
        const uint32_t counts[5] = {c.len, c.uncorrected_len, c.lstrip, c.rstrip, c.lqseq_total_length};
        memcpy(rq.counts, counts, sizeof(counts));
    });
    size_t n_words = 0, n_wins = 0;
    for (const CnsReq &rq : reqs) n_words += rq.words.size(), n_wins += rq.wins.size();
    uint32_t *bw = (uint32_t *)malloc(std::max<size_t>(1, n_words) * sizeof(uint32_t));
    uint32_t *rw = (uint32_t *)malloc(std::max<size_t>(1, n_wins) * sizeof(uint32_t));
    if (!bw || !rw) {
        free(bw), free(rw);
        return -3;
    }
    size_t at_w = 0, at_r = 0;
    for (int i = 0; i < n; i++) {
        const CnsReq &rq = reqs[(size_t)i];
        ndgpu_cns_result &o = res[i];
        memset(&o, 0, sizeof(o));
        CnsCounts c;
        c.len = o.len = rq.counts[0], c.uncorrected_len = o.uncorrected_len = rq.counts[1], c.lstrip = o.lstrip = rq.counts[2];
        c.rstrip = o.rstrip = rq.counts[3], c.lqseq_total_length = o.lqseq_total_length = rq.counts[4];
        o.ok = cns_verdict(c, jobs[i].min_error_corrected_ratio) ? 1 : 0;
        o.n_regions = (uint32_t)(rq.wins.size() / 2);
        o.base_off = at_w, o.region_off = at_r / 2;
        if (!rq.words.empty()) memcpy(bw + at_w, rq.words.data(), rq.words.size() * sizeof(uint32_t));
        if (!rq.wins.empty()) memcpy(rw + at_r, rq.wins.data(), rq.wins.size() * sizeof(uint32_t));
        at_w += rq.words.size(), at_r += rq.wins.size();
    }
    *bases = bw, *regions = rw;
    return 0;
}

// The loop behind a batch of walks in any of its three forms.  Mode 0 is ndgpu_cns_windows_batch itself, called for the mode-0 jobs of
// the batch; modes 1 and 2 go through K21 (DeviceAligner::run_cns_walk) or -- flags bit 0, or a walk the kernel declines -- through
// cns_kmer_host / cns_fast_host.  The verdict, the length and the identity are computed here from either's counters.
int ndgpu_cns_walk_batch(const ndgpu_cns_walk_job *jobs, int n, int flags, ndgpu_cns_walk_result *res, uint32_t **bases, uint32_t **regions,
                         char **seqs) {
    if (n == 0) return 0;
    if (n < 0 || !jobs || !res || !bases || !regions || !seqs) return -2;
    size_t total = 0, seed_total = 0;
    std::vector<ndgpu_cns_job> raw;
    std::vector<size_t> walk_ids;
    for (int i = 0; i < n; i++) {
        const ndgpu_cns_walk_job &j = jobs[i];
        if (j.n && !j.steps) return -2;
        if (j.mode < 0 || j.mode > 2) return -2;
        if (j.mode == 1 && !j.seed) return -2;
        for (uint32_t k = 0; k < j.n; k++) {
            const ndgpu_walk_step &s = j.steps[k];
            if (s.base == 4) continue;
            if (s.cov == 0 || s.base > 5 || s.t_pos < 0 || s.t_pos > (1 << 21) - 2) return -2;
            if (j.mode == 1 && (uint32_t)s.t_pos >= j.seed_len) return -2;
        }
        if (j.mode == 0) raw.push_back(ndgpu_cns_job{j.steps, j.n, j.min_cov, j.lq_max_len, j.min_error_corrected_ratio});
        else {
            walk_ids.push_back((size_t)i);
            total += j.n;
            if (j.mode == 1) seed_total += j.seed_len;
        }
    }
    // the mode-0 jobs: the existing entry's answer, word for word
    std::vector<ndgpu_cns_result> raw_res(raw.size());
    uint32_t *raw_bases = nullptr, *raw_regions = nullptr;
    if (!raw.empty()) {
        const int rc = ndgpu_cns_windows_batch(raw.data(), (int)raw.size(), flags, raw_res.data(), &raw_bases, &raw_regions);
        if (rc != 0) return rc;
    }
    struct Keep {   // (frees the two blocks on every way out)
        uint32_t *a, *b;
        ~Keep() { free(a), free(b); }
    } keep{raw_bases, raw_regions};
    std::vector<PathStep> steps(total);
    std::vector<uint8_t> codes(seed_total);
    std::vector<CnsWalkReq> reqs(walk_ids.size());
    for (size_t r = 0, at = 0, sat = 0; r < reqs.size(); r++) {
        const ndgpu_cns_walk_job &j = jobs[walk_ids[r]];
        for (uint32_t k = 0; k < j.n; k++) {
            PathStep &d = steps[at + k];
            d.t_pos = j.steps[k].t_pos, d.delta = 0, d.base = j.steps[k].base, d.link = j.steps[k].link, d.cov = j.steps[k].cov;
        }
        CnsWalkReq &rq = reqs[r];
        rq.steps = steps.data() + at, rq.n = j.n, rq.min_cov = j.min_cov, rq.mode = j.mode;
        at += j.n;
        if (j.mode == 1) {
            for (uint32_t k = 0; k < j.seed_len; k++) codes[sat + k] = cns_base_code((unsigned char)j.seed[k]);
            rq.seed_codes = codes.data() + sat, rq.seed_len = j.seed_len;
            sat += j.seed_len;
        }
    }
    if (!(flags & 1) && !reqs.empty()) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
            fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_cns_walk_batch runs on the device unless flags bit 0 is set\n");
            return -1;
        }
        std::vector<std::pair<size_t, size_t>> todo{{0, reqs.size()}};   // (out of device memory: the range is halved until it fits)
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            try {
                HipBackend be(0, 1);
                be.run_cns_walk(reqs.data() + a, b - a);
            } catch (const DeviceOom &) {
                DeviceAligner::context(0).release_memory();
                DeviceAligner::forget_sizes();
                if (b - a <= 1) return -3;
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    host_each(reqs.size(), effective_cpus() <= 1 || reqs.size() <= 1, effective_cpus(), reqs.size(), false, [&](size_t r) {
        CnsWalkReq &rq = reqs[r];
        if (rq.done) return;
        if (rq.mode == 1) {
            std::vector<CnsWindow> wins;
            CnsCounts c;
            cns_kmer_host(rq.steps, rq.n, rq.seed_codes, rq.min_cov, rq.words, wins, c);
            rq.wins.clear();
            for (const CnsWindow &w : wins) rq.wins.push_back(w.start), rq.wins.push_back(w.end);
            rq.len = c.len, rq.lqseq_total_length = c.lqseq_total_length;
        } else {
            CnsFastOut o;
            cns_fast_host(rq.steps, rq.n, rq.min_cov, o);
            rq.lq_m = o.lq_m, rq.hq_m = o.hq_m, rq.lqseq_total_length = o.lq_total_len, rq.len = o.out_len;
            rq.seq.swap(o.seq);
        }
    });
    size_t n_words = 0, n_wins = 0, n_seq = 0;
    for (const ndgpu_cns_result &r : raw_res) n_words += r.len, n_wins += 2 * (size_t)r.n_regions;
    for (const CnsWalkReq &rq : reqs) n_words += rq.words.size(), n_wins += rq.wins.size(), n_seq += rq.seq.size();
    uint32_t *bw = (uint32_t *)malloc(std::max<size_t>(1, n_words) * sizeof(uint32_t));
    uint32_t *rw = (uint32_t *)malloc(std::max<size_t>(1, n_wins) * sizeof(uint32_t));
    char *sw = (char *)malloc(std::max<size_t>(1, n_seq));
    if (!bw || !rw || !sw) {
        free(bw), free(rw), free(sw);
        return -3;
    }
    size_t at_w = 0, at_r = 0, at_s = 0, i_raw = 0, i_walk = 0;
    for (int i = 0; i < n; i++) {
        ndgpu_cns_walk_result &o = res[i];
        memset(&o, 0, sizeof(o));
        if (jobs[i].mode == 0) {
            const ndgpu_cns_result &r = raw_res[i_raw++];
            o.len = r.len, o.uncorrected_len = r.uncorrected_len, o.lstrip = r.lstrip, o.rstrip = r.rstrip;
            o.lqseq_total_length = r.lqseq_total_length, o.ok = r.ok, o.n_regions = r.n_regions;
            o.base_off = at_w, o.region_off = at_r / 2;
            if (r.len) memcpy(bw + at_w, raw_bases + r.base_off, (size_t)r.len * sizeof(uint32_t));
            if (r.n_regions) memcpy(rw + at_r, raw_regions + 2 * r.region_off, 2 * (size_t)r.n_regions * sizeof(uint32_t));
            at_w += r.len, at_r += 2 * (size_t)r.n_regions;
            continue;
        }
        const CnsWalkReq &rq = reqs[i_walk++];
        o.base_off = at_w, o.region_off = at_r / 2, o.seq_off = at_s;
        if (rq.mode == 1) {
            CnsCounts c;
            c.len = o.len = rq.len, c.lqseq_total_length = o.lqseq_total_length = rq.lqseq_total_length;
            o.ok = cns_kmer_verdict(c, jobs[i].min_error_corrected_ratio) ? 1 : 0;
            o.n_regions = (uint32_t)(rq.wins.size() / 2);
            if (!rq.words.empty()) memcpy(bw + at_w, rq.words.data(), rq.words.size() * sizeof(uint32_t));
            if (!rq.wins.empty()) memcpy(rw + at_r, rq.wins.data(), rq.wins.size() * sizeof(uint32_t));
            at_w += rq.words.size(), at_r += rq.wins.size();
        } else {
            o.len = cns_fast_len(rq.lq_m, rq.hq_m);
            o.identity = cns_fast_identity(rq.lqseq_total_length, o.len);
            o.lq_total_len = rq.lqseq_total_length;
            o.seq_len = (uint32_t)rq.seq.size();
            o.ok = 1;
            if (!rq.seq.empty()) memcpy(sw + at_s, rq.seq.data(), rq.seq.size());
            at_s += rq.seq.size();
        }
    }
    *bases = bw, *regions = rw, *seqs = sw;
    return 0;
}

// The end of a batch of piles: K24 (DeviceAligner::run_splice) or -- flags bit 0, or a job the runtime declines -- splice_host and
// ssr_trim_host.  Length and identity are formed here from either's integers (splice_finish of nd_splice.h).
int ndgpu_splice_batch(const ndgpu_splice_job *jobs, int n, int flags, ndgpu_splice_result *res, char **seqs) {
    if (n == 0) return 0;
    if (n < 0 || !jobs || !res || !seqs) return -2;
    size_t n_reg = 0;
    for (int i = 0; i < n; i++) {
        const ndgpu_splice_job &j = jobs[i];
        if ((j.n_words && !j.words) || (j.n_regions && !j.regions)) return -2;
        if ((uint64_t)j.lstrip + j.rstrip > j.n_words) return -2;
        for (uint32_t k = j.lstrip + 1; k < j.n_words - j.rstrip; k++)
            if ((j.words[k] >> 8) < (j.words[k - 1] >> 8)) return -2;
        for (uint32_t k = 0; k < j.n_regions; k++)
            if (j.regions[k].start > j.regions[k].end || (j.regions[k].sudoseed_len && !j.regions[k].sudoseed)) return -2;
        n_reg += j.n_regions;
    }
    std::vector<SpliceRegion> regs(n_reg);
    std::vector<SpliceReq> reqs((size_t)n);
    for (size_t i = 0, at = 0; i < (size_t)n; i++) {
        const ndgpu_splice_job &j = jobs[i];
        for (uint32_t k = 0; k < j.n_regions; k++) {
            SpliceRegion &r = regs[at + k];
            r.start = j.regions[k].start, r.end = j.regions[k].end, r.len = j.regions[k].len;
            r.sudoseed_len = j.regions[k].sudoseed_len, r.sudoseed = j.regions[k].sudoseed;
        }
        SpliceReq &rq = reqs[i];
        rq.words = j.words, rq.len = j.n_words, rq.lstrip = j.lstrip, rq.rstrip = j.rstrip;
        rq.regions = regs.data() + at, rq.n_regions = j.n_regions, rq.hifi = j.read_type == 3;
        at += j.n_regions;
    }
    std::vector<SpliceReq *> ptr(reqs.size());
    for (size_t i = 0; i < reqs.size(); i++) ptr[i] = &reqs[i];
    if (!(flags & 1)) {
        int n_dev = 0;
        if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
            fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_splice_batch runs on the device unless flags bit 0 is set\n");
            return -1;
        }
        std::vector<std::pair<size_t, size_t>> todo{{0, reqs.size()}};   // (out of device memory: the range is halved until it fits)
        while (!todo.empty()) {
            const auto [a, b] = todo.back();
            todo.pop_back();
            try {
                HipBackend be(0, 1);
                (void)be.run_splice(ptr.data() + a, b - a);
            } catch (const DeviceOom &) {
                DeviceAligner::context(0).release_memory();
                DeviceAligner::forget_sizes();
                if (b - a <= 1) return -3;
                todo.push_back({a + (b - a) / 2, b});
                todo.push_back({a, a + (b - a) / 2});
            }
        }
    }
    std::vector<SpliceAnswer> ans((size_t)n);
    host_each(reqs.size(), effective_cpus() <= 1 || reqs.size() <= 1, effective_cpus(), reqs.size(), false, [&](size_t i) {
        SpliceReq &rq = reqs[i];
        SpliceAnswer &a = ans[i];
        if (!rq.done) {
            splice_answer_host(rq.words, rq.len, rq.lstrip, rq.rstrip, rq.regions, rq.n_regions, rq.hifi, a);
            return;
        }
        // the device's integers; the host forms the float
        a.out_len = rq.out_len, a.lq_m = rq.lq_m, a.hq_m = rq.hq_m, a.lq_i = rq.lq_i, a.lq_total_len = rq.lq_total_len;
        a.clip_s = rq.clip_s, a.clip_e = rq.clip_e, a.trimmed = rq.trimmed;
        const unsigned len0 = splice_len(rq.lq_m, rq.hq_m, rq.code == 2u);
        a.identity = splice_identity(rq.lq_total_len, len0, rq.code == 2u);
        a.len = rq.code ? rq.code : (uint32_t)rq.seq.size();
        a.seq.swap(rq.seq);
    });
    size_t n_seq = 0;
    for (const SpliceAnswer &a : ans) n_seq += a.seq.size();
    char *sw = (char *)malloc(std::max<size_t>(1, n_seq));
    if (!sw) return -3;
    size_t at = 0;
    for (int i = 0; i < n; i++) {
        const SpliceAnswer &a = ans[(size_t)i];
        ndgpu_splice_result &o = res[i];
        memset(&o, 0, sizeof(o));
        o.len = a.len, o.lq_total_len = a.lq_total_len, o.identity = a.identity, o.out_len = a.out_len, o.lq_m = a.lq_m, o.hq_m = a.hq_m;
        o.lq_i = a.lq_i, o.clip_s = a.clip_s, o.clip_e = a.clip_e;
        o.seq_len = (uint32_t)a.seq.size(), o.seq_off = at;
        if (!a.seq.empty()) memcpy(sw + at, a.seq.data(), a.seq.size());
        at += a.seq.size();
    }
    *seqs = sw;
    return 0;
}

// ---- batched global alignment: align() / align_hq() for many pairs in one call, CIGARs built on the device (K15) ----
namespace {
struct AlnBatchSrc {            // where job i's bases are, for the strings flag
    const char *q, *t;
    std::string q_own, t_own;   // DB form: host copies of the two windows
};

// `run`: K7 / K8a + K15 (or, flags bit 0, the old tail and the host's run-length loop) over jobs[0, n); everything the caller sees
// is written only after the whole batch is done
int align_batch_common(std::vector<AlnJob> &jobs, const uint32_t *db_pool, int flags, ndgpu_aln_result *res, uint32_t **cigar, char **q_aln,
                       char **t_aln, const std::function<void(size_t, AlnBatchSrc &)> &source) {
    const size_t n = jobs.size();
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0) {
        fprintf(stderr, "[ndgpu] FATAL: no HIP device visible: ndgpu_align_batch aligns on the device\n");
        return -1;
    }
    std::vector<AlnJob *> ptr(n);
    for (size_t i = 0; i < n; i++) ptr[i] = &jobs[i];
    std::vector<AlnRunsResult> sum(n);
    std::vector<uint32_t> runs;
    const int threads = effective_cpus();
    // (out of device memory: the range is halved until it fits; ranges are served in job order, so the runs stay in job order)
    std::vector<std::pair<size_t, size_t>> todo{{0, n}};
    while (!todo.empty()) {
        const auto [a, b] = todo.back();
        todo.pop_back();
        const size_t runs_before = runs.size();
        try {
            HipBackend be(0, threads, db_pool);
            if (flags & 1) {
                be.run_align(ptr.data() + a, b - a);
                for (size_t i = a; i < b; i++) {
                    sum[i] = AlnRunsResult();
                    sum[i].run_off = runs.size();
                    if (jobs[i].status == ALN_NONE) continue;
                    aln_runs_host(jobs[i].ops.data(), jobs[i].ops.size(), sum[i], runs);
                    sum[i].status = jobs[i].status, sum[i].q_used = (uint32_t)jobs[i].q_used, sum[i].t_used = (uint32_t)jobs[i].t_used;
                    std::vector<uint8_t>().swap(jobs[i].ops);
                }
            } else {
                std::vector<uint32_t> part;
                be.run_align_runs(ptr.data() + a, b - a, sum.data() + a, part);
                for (size_t i = a; i < b; i++) sum[i].run_off += runs.size();
                runs.insert(runs.end(), part.begin(), part.end());
            }
        } catch (const DeviceOom &) {
            DeviceAligner::context(0).release_memory();
            DeviceAligner::forget_sizes();
            runs.resize(runs_before);
            if (b - a <= 1) return -3;
            todo.push_back({a + (b - a) / 2, b});
            todo.push_back({a, a + (b - a) / 2});
        }
    }
    // the two gapped strings exactly as align() writes them, rebuilt from the runs: job i's at the sum of (aln_len + 1) of the jobs before it
    char *qs = nullptr, *ts = nullptr;
    if (flags & 2) {
        std::vector<uint64_t> at(n + 1, 0);
        for (size_t i = 0; i < n; i++) at[i + 1] = at[i] + sum[i].aln_len + 1;
        qs = (char *)malloc((size_t)at[n] + 1), ts = (char *)malloc((size_t)at[n] + 1);
        if (!qs || !ts) {
            free(qs), free(ts);
            return -3;
        }
        host_each(n, threads <= 1 || n <= 1, threads, n, false, [&](size_t i) {
            const AlnRunsResult &r = sum[i];
            char *qa = qs + at[i], *ta = ts + at[i];
            size_t c = 0;
            if (r.status != ALN_NONE) {
                AlnBatchSrc src;
                source(i, src);
                // (the > 250-gap abort keeps the last two columns: their bases end at q_used / t_used)
                size_t qi = r.status == ALN_GAP_ABORT ? r.q_used - (r.n_match + r.n_ins) : 0;
                size_t ti = r.status == ALN_GAP_ABORT ? r.t_used - (r.n_match + r.n_del) : 0;
                for (uint32_t k = 0; k < r.n_runs; k++) {
                    const uint32_t w = runs[r.run_off + k], op = w & 15u;
                    for (uint32_t len = w >> 4; len; len--, c++) {
                        ta[c] = op == 1u ? '-' : src.t[ti++];
                        qa[c] = op == 2u ? '-' : src.q[qi++];
                    }
                }
            }
            qa[c] = ta[c] = '\0';
        });
    }
    uint32_t *cg = (uint32_t *)malloc(std::max<size_t>(1, runs.size()) * sizeof(uint32_t));
    if (!cg) {
        free(qs), free(ts);
        return -3;
    }
    if (!runs.empty()) memcpy(cg, runs.data(), runs.size() * sizeof(uint32_t));
    for (size_t i = 0; i < n; i++) {
        const AlnRunsResult &r = sum[i];
        ndgpu_aln_result &o = res[i];
        o.status = r.status, o.aln_len = r.aln_len, o.q_used = r.q_used, o.t_used = r.t_used;
        o.n_match = r.n_match, o.n_ins = r.n_ins, o.n_del = r.n_del, o.max_gap_run = r.max_gap_run;
        o.n_cigar = r.n_runs, o.cigar_off = r.run_off;
    }
    *cigar = cg;
    if (flags & 2) *q_aln = qs, *t_aln = ts;
    return 0;
}
}  // namespace

int ndgpu_align_batch(const ndgpu_aln_job *jobs, int n, int flags, ndgpu_aln_result *res, uint32_t **cigar, char **q_aln, char **t_aln) {
    if (n == 0) return 0;
    if (n < 0 || !jobs || !res || !cigar || ((flags & 2) && (!q_aln || !t_aln))) return -2;
    for (int i = 0; i < n; i++) {
        const ndgpu_aln_job &j = jobs[i];
        if (j.q_len < 0 || j.t_len < 0 || (int64_t)j.q_len + j.t_len >= (1 << 28) || (!j.q && j.q_len) || (!j.t && j.t_len)) return -2;
    }
    std::vector<AlnJob> aj((size_t)n);
    for (int i = 0; i < n; i++) aj[i].q = jobs[i].q, aj[i].q_len = jobs[i].q_len, aj[i].t = jobs[i].t, aj[i].t_len = jobs[i].t_len, aj[i].hq = jobs[i].hq != 0;
    return align_batch_common(aj, nullptr, flags, res, cigar, q_aln, t_aln, [&](size_t i, AlnBatchSrc &s) { s.q = jobs[i].q, s.t = jobs[i].t; });
}

int ndgpu_align_db_batch(ndgpu_db *h, const ndgpu_aln_dbjob *jobs, int n, int flags, ndgpu_aln_result *res, uint32_t **cigar, char **q_aln,
                         char **t_aln) {
    if (n == 0) return 0;
    if (n < 0 || !h || !h->db || !h->dev_pool || !jobs || !res || !cigar || ((flags & 2) && (!q_aln || !t_aln))) return -2;
    const ReadDb &db = *h->db;
    auto inside = [&](uint32_t r, uint32_t s, uint32_t e) { return r < db.n_reads() && s <= e && e < db.length(r); };
    for (int i = 0; i < n; i++) {
        const ndgpu_aln_dbjob &j = jobs[i];
        if (!inside(j.q_read, j.q_start, j.q_end) || !inside(j.t_read, j.t_start, j.t_end)) return -2;
        if ((uint64_t)(j.q_end - j.q_start) + (j.t_end - j.t_start) + 2 >= (1u << 28)) return -2;
    }
    std::vector<AlnJob> aj((size_t)n);
    for (int i = 0; i < n; i++) {
        const ndgpu_aln_dbjob &j = jobs[i];
        aj[i].q_len = (int)(j.q_end - j.q_start + 1), aj[i].t_len = (int)(j.t_end - j.t_start + 1), aj[i].hq = j.hq != 0;
        aj[i].q_dev = db.window_offset(j.q_read, j.q_start, j.q_end, j.q_rev != 0);
        aj[i].t_dev = db.window_offset(j.t_read, j.t_start, j.t_end, j.t_rev != 0);
    }
    return align_batch_common(aj, h->dev_pool, flags, res, cigar, q_aln, t_aln, [&](size_t i, AlnBatchSrc &s) {
        const ndgpu_aln_dbjob &j = jobs[i];
        s.q_own = db.window(j.q_read, j.q_start, j.q_end, j.q_rev != 0), s.t_own = db.window(j.t_read, j.t_start, j.t_end, j.t_rev != 0);
        s.q = s.q_own.data(), s.t = s.t_own.data();
    });
}

void ndgpu_get_stats(ndgpu_stats *o) {
    RuntimeStats s = DeviceAligner::total_stats();
    o->tasks = s.tasks;
    o->wide_tasks = s.wide_tasks;
    o->cells = s.cells;
    o->d_steps = s.d_steps;
    o->trace_bits = s.trace_bits;
    o->columns = s.columns;
    o->pool_bases = s.pool_bases;
    o->seq_bases = s.seq_bases;
    o->max_band = s.max_band;
    o->forward_launches = s.forward_launches;
    o->forward_ms = s.forward_ms;
    o->traceback_ms = s.traceback_ms;
    o->tags_ms = s.tags_ms;
    o->links_ms = s.links_ms;
    o->score_ms = s.score_ms;
    o->extract_ms = s.extract_ms;
    o->piles = s.piles;
    o->tags = s.tags;
    o->cells_msa = s.cells_msa;
    o->path_items = s.path_items;
    o->links = s.links;
    o->score_launches = s.score_launches;
    o->backtrack_ms = s.backtrack_ms;
    o->score_segments = s.score_segments;
    o->score_repairs = s.score_repairs;
    o->score_slow_piles = s.score_slow_piles;
    o->trace_words = s.trace_words;
    o->lq_rounds = s.lq_rounds;
    o->lq_declined = s.lq_declined;
    o->lq_ms = s.lq_ms;
    o->allocs = s.allocs, o->alloc_ms = s.alloc_ms, o->level_allocs = s.level_allocs, o->level_ms = s.level_ms;
    o->traceback_launches = s.traceback_launches, o->lq_launches = s.lq_launches, o->lq_columns = s.lq_columns;
    o->lq_aln_columns = s.lq_aln_columns, o->lq_bases = s.lq_bases, o->lq_out = s.lq_out;
    o->lq_jobs = s.lq_jobs, o->lq_repairs = s.lq_repairs;
    o->tb_tasks = s.tb_tasks, o->tb_walkers = s.tb_walkers, o->tb_fallbacks = s.tb_fallbacks;
    o->poa_jobs = s.poa_jobs, o->poa_declined = s.poa_declined, o->poa_rounds = s.poa_rounds, o->poa_launches = s.poa_launches;
    o->poa_cells = s.poa_cells, o->poa_ms = s.poa_ms;
    o->rank_jobs = s.rank_jobs, o->rank_tail = s.rank_tail, o->rank_launches = s.rank_launches, o->rank_ms = s.rank_ms;
    o->aln_batch_jobs = s.aln_batch_jobs, o->aln_batch_launches = s.aln_batch_launches, o->aln_batch_runs = s.aln_batch_runs;
    o->aln_batch_ms = s.aln_batch_ms;
    o->poa_resident_jobs = s.poa_resident_jobs, o->poa_resident_declined = s.poa_resident_declined;
    o->poa_graph_launches = s.poa_graph_launches, o->poa_graph_ms = s.poa_graph_ms;
    o->poa_h2d_bytes = s.poa_h2d_bytes, o->poa_d2h_bytes = s.poa_d2h_bytes;
    o->cns_jobs = s.cns_jobs, o->cns_declined = s.cns_declined, o->cns_launches = s.cns_launches, o->cns_regions = s.cns_regions;
    o->cns_ms = s.cns_ms, o->cns_d2h_bytes = s.cns_d2h_bytes, o->walk_d2h_bytes = s.walk_d2h_bytes;
}

void ndgpu_reset_stats(void) { DeviceAligner::reset_all_stats(); }

void ndgpu_get_cns_mode_stats(ndgpu_cns_mode_stats *o) {
    if (!o) return;
    const RuntimeStats s = DeviceAligner::total_stats();
    o->hifi_jobs = s.cnsw_hifi_jobs, o->hifi_declined = s.cnsw_hifi_declined, o->hifi_regions = s.cnsw_hifi_regions;
    o->fast_jobs = s.cnsw_fast_jobs, o->fast_declined = s.cnsw_fast_declined, o->launches = s.cnsw_launches;
    o->ms = s.cnsw_ms, o->d2h_bytes = s.cnsw_d2h_bytes;
}

void ndgpu_get_phase_stats(ndgpu_phase_stats *o) {
    if (!o) return;
    const RuntimeStats s = DeviceAligner::total_stats();
    o->piles = s.phase_piles, o->regions = s.phase_regions, o->pass2_piles = s.phase_pass2, o->tail_passes = s.phase_tail;
    for (int k = 0; k < 4; k++) o->kind[k] = s.phase_kind[k];
    for (int k = 0; k < 5; k++) o->declined[k] = s.phase_declined[k];
    o->launches = s.phase_launches, o->ms = s.phase_ms;
    o->d2h_record_bytes = s.phase_d2h_records, o->d2h_string_bytes = s.phase_d2h_strings;
    o->seed_lower = s.phase_lower;
}

void ndgpu_get_splice_stats(ndgpu_splice_stats *o) {
    if (!o) return;
    const RuntimeStats s = DeviceAligner::total_stats();
    o->jobs = s.splice_jobs, o->declined = s.splice_declined, o->launches = s.splice_launches;
    o->h2d_bytes = s.splice_h2d_bytes, o->d2h_bytes = s.splice_d2h_bytes, o->trimmed = s.splice_trimmed, o->ms = s.splice_ms;
}

uint64_t ndgpu_release_memory(void) {
    size_t f0 = 0, f1 = 0, t = 0;
    (void)hipMemGetInfo(&f0, &t);
    join_reapers();
    for (int c = 0; c < DeviceAligner::kMaxContexts; c++)
        if (DeviceAligner *d = DeviceAligner::peek(c)) (void)d->release_memory_if_idle();  // a context with a batch open keeps its buffers
    (void)hipMemGetInfo(&f1, &t);
    return f1 > f0 ? (uint64_t)(f1 - f0) : 0;
}

void ndgpu_reserve_device_memory(uint64_t bytes) { DeviceAligner::reserve_device_memory(bytes); }

int ndgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

}  // extern "C"
