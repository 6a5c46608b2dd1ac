// The phasing and ranking of a HiFi pile's low-quality-region candidates (generate_lqseqs_from_tags_kmer and its helpers,
// lib/nextcorrect.c:512-737, 740-1008), from the candidates as laid out up to the sort by score, stated once on the host: the engine
// (Impl::lqseqs_from_candidates_kmer of consensus.cpp), the host flag of ndgpu_hifi_phase_batch and the tests share this statement;
// K22 (hifi_phase_kernel and hifi_phase_rank_kernel, lq_kernels.hip) is its device form.  Pure: no device, no environment.
// What follows the records -- the selection loop with its double comparisons, indexe, the < 20000 test, the POA hand-over,
// max_aln_length -- stays with the caller.
// (Inline, standard headers only: a stand-alone sanitizer program of the tests includes this header and nothing else.)
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace ndgpu {

constexpr int kPhaseCanMax = 40;    // LQ_CAN_MAX: candidates of a region
constexpr int kPhaseSeqMax = 30;    // LQSEQ_MAX_CAN_COUNT
enum : uint8_t {
    kPhaseEmpty = 0,     // the region had no candidates
    kPhaseDropped = 1,   // lq.len = 0: after one of the two trims (:918, :928), or every candidate's read was phased away (:876)
    kPhaseSeed = 2,      // a candidate becomes the pseudo-seed, lq.len = -2
    kPhaseRanked = 3     // the region reaches the selection loop
};

// One region's outcome: 128 bytes.  perm and kscore describe lq.seqs as the rule leaves it, every position of it -- also those beyond
// n, which the swaps, the sort and the trims moved out of the way: perm[j] is the input index of the candidate at position j,
// kscore[j] its score as left by the last step that wrote it (the ranking's sum with the tail pass included).  Entries from n_cand on
// are 0, and an empty region is all 0.
struct PhaseRecord {
    uint8_t kind;        // kPhase*
    uint8_t lower;       // kPhaseSeed: kscore < len / 2, the pseudo-seed goes to lower case
    uint8_t indexs;      // as the phasing left it (0, 1, 2)
    uint8_t tail;        // kPhaseRanked: the tail windows were ranked too (seqs[0].len > 100)
    int16_t n;           // the final lq.len: -2 (seed), 0 (dropped, empty), or the number of ranked candidates
    uint8_t seed;        // kPhaseSeed: the input index of the candidate ...
    uint8_t seed_pos;    // ... and its position: perm[seed_pos] == seed
    uint8_t perm[kPhaseCanMax];
    uint16_t kscore[kPhaseCanMax];
};
static_assert(sizeof(PhaseRecord) == 128, "the device writes this record as it stands");

struct PhaseRegionIn {
    uint32_t start, end;          // inclusive seed columns
    int n_cand;                   // 0..40
    const char *const *seq;       // the candidates' bytes ...
    const uint16_t *len;          // ... lengths ...
    const uint16_t *src;          // ... and source reads (< n_aligned)
};
struct PhasePileOut {
    uint8_t has_heter = 0, pass2 = 0;
};

namespace phase_detail {

struct Seq {
    uint16_t order, kscore, len;
    uint8_t idx;
    const char *seq;
};
struct Region {
    uint32_t start, end;
    int len, n_cand;
    uint8_t indexs;
    Seq seqs[kPhaseCanMax];
};
struct Phs {
    uint16_t d = 0, s = 0;   // (wrap at 65,536, as the reference's)
    int del = 0;
};

inline bool same_seq(const Seq &a, const Seq &b) { return a.len == b.len && (a.len == 0 || memcmp(a.seq, b.seq, a.len) == 0); }

// A/a 0, T/t 1, G/g 2, C/c 3, N 5, M 6, any other byte 4 (consensus.cpp: BaseLut)
inline unsigned code(char ch) {
    const unsigned c = (unsigned char)ch, u = c & 0xdfu;
    return u == 'A' ? 0u : u == 'T' ? 1u : u == 'G' ? 2u : u == 'C' ? 3u : c == 'N' ? 5u : c == 'M' ? 6u : 4u;
}

// the partition by swaps of remove_differ_len and remove_differ_phase_lqseq (:524-537, :599-609): not stable
inline void compact_flagged(Region &lq, const int8_t *dif) {
    int j, k;
    for (k = lq.len, j = 0; j < lq.len && j < k; j++)
        if (dif[j])
            for (k--; k > j; k--)
                if (!dif[k]) {
                    std::swap(lq.seqs[j], lq.seqs[k]);
                    break;
                }
    lq.len = k;
}

inline int remove_differ_len(Region &lq) {  // :512-539
    int s, j;
    const int k = (int)(lq.end - lq.start + 1);
    const int offset = std::min(std::max(30, k / 10), k / 3);
    int8_t dif[kPhaseCanMax] = {0};
    for (j = s = 0; j < lq.len; j++) {
        if (lq.seqs[j].len + offset >= k && lq.seqs[j].len <= k + offset) s++;
        else dif[j] = 1;
    }
    if (s != lq.len && (s >= lq.len / 2 || (s >= lq.len / 3 && s >= 3))) compact_flagged(lq, dif);
    return s;
}

inline void select_most2(Region &lq, int len, int *m1, int *m2) {  // :632-653
    int j, k;
    int8_t used[kPhaseCanMax] = {0};
    for (*m1 = *m2 = j = 0; j < std::min(lq.len, len); j++) {
        lq.seqs[j].kscore = 1;
        if (used[j]) continue;
        for (k = j + 1; k < lq.len; k++)
            if (same_seq(lq.seqs[j], lq.seqs[k])) {
                used[k] = 1;
                lq.seqs[j].kscore++;
            }
        if (lq.seqs[j].kscore > lq.seqs[*m1].kscore ||
            (lq.seqs[j].kscore == lq.seqs[*m1].kscore && lq.seqs[j].order < lq.seqs[*m1].order)) {
            *m2 = *m1;
            *m1 = j;
        } else if (*m2 == *m1 || lq.seqs[j].kscore > lq.seqs[*m2].kscore) {
            *m2 = j;
        }
    }
}

inline void select_most2_with_kscore(Region &lq, int len, int *m1, int *m2) {  // :656-668
    int j;
    for (*m1 = *m2 = j = 0; j < std::min(lq.len, len); j++) {
        if (lq.seqs[j].kscore > lq.seqs[*m1].kscore ||
            (lq.seqs[j].kscore == lq.seqs[*m1].kscore && lq.seqs[j].order < lq.seqs[*m1].order)) {
            *m2 = *m1;
            *m1 = j;
        } else if (*m2 == *m1 || lq.seqs[j].kscore > lq.seqs[*m2].kscore) {
            *m2 = j;
        }
    }
}

inline void run_ends(const Seq &q, int *s, int *e) {  // :678-683
    const int n = (int)q.len;
    *s = 0;
    while (*s + 1 < n && q.seq[*s] == q.seq[*s + 1]) (*s)++;
    *e = n - 1;
    while (*e > 0 && q.seq[*e - 1] == q.seq[*e]) (*e)--;
}
inline int homo_end_same(const Seq &a, const Seq &b) {  // :684-697
    int as, ae, bs, be;
    run_ends(a, &as, &ae);
    run_ends(b, &bs, &be);
    if (ae <= as && be <= bs) return 1;
    if (ae - as != be - bs) return 0;
    for (int i = 0; i <= ae - as; i++)
        if (a.seq[i + as] != b.seq[i + bs]) return 0;
    return 1;
}
inline int prefixhomo_same(const Seq &a, const Seq &b) {  // :699-714
    int i = 0, j = 0;
    const int na = (int)a.len, nb = (int)b.len;
    while (i < na && j < nb) {
        if (a.seq[i] != b.seq[j]) return 0;
        while (i + 1 < na && a.seq[i] == a.seq[i + 1]) i++;
        while (j + 1 < nb && b.seq[j] == b.seq[j + 1]) j++;
        i++;
        j++;
    }
    return 1;
}
// :716-737.  Where the longer string has more than twice the shorter one's bytes the reference's second loop reads in front of the
// shorter string; such a byte counts as a mismatch here (and in K22).
inline int trim_endssr_same(const Seq &x, const Seq &y) {
    const Seq *a = &x, *b = &y;
    if (a->len < b->len) std::swap(a, b);
    const int na = (int)a->len, nb = (int)b->len;
    int i;
    for (i = 0; i < nb; i++)
        if (a->seq[i] != b->seq[i]) return 0;
    for (int j = na - 1; j >= i; j--) {
        const int at = nb - (na - j);
        if (at < 0 || a->seq[j] != b->seq[at]) return 0;
    }
    return 1;
}

// count_kmers with c = LQ_CAN_MAX and count_kscore (:281-337) over the head or the tail windows: every sequence of the region is
// counted, every sequence scored with the sum of its own k-mers' counts
inline void rank_pass(Region &lq, std::vector<uint16_t> &bins, int from_tail) {
    constexpr int kK = 8, kRange = 40;
    std::vector<uint16_t> touched;
    for (int pass = 0; pass < 2; pass++)
        for (int j = 0; j < lq.len; j++) {
            Seq &s = lq.seqs[j];
            if (pass) s.kscore = 0;
            if (s.len < kK) continue;
            const int off = from_tail && s.len > kRange ? s.len - kRange : 0;
            const int n = std::min<int>(s.len, kRange) - kK;
            uint16_t km = 0;
            for (int k = 0; k < n; k++) {
                if (k) km = (uint16_t)(km << 2 | code(s.seq[off + k + kK - 1]));
                else
                    for (int x = 0; x < kK; x++) km = (uint16_t)(km << 2 | code(s.seq[off + x]));
                if (pass) s.kscore = (uint16_t)(s.kscore + bins[km]);
                else if (bins[km]++ == 0) touched.push_back(km);
            }
        }
    for (uint16_t t : touched) bins[t] = 0;
}

inline void write_record(const Region &lq, PhaseRecord &o, uint8_t kind, int n) {
    o.kind = kind;
    o.indexs = lq.indexs;
    o.n = (int16_t)n;
    for (int j = 0; j < lq.n_cand; j++) o.perm[j] = lq.seqs[j].idx, o.kscore[j] = lq.seqs[j].kscore;
}

}  // namespace phase_detail

// regs: the pile's regions in order; src < n_aligned (n_aligned >= 1).  out: one record per region.
inline void hifi_phase_host(unsigned n_aligned, const PhaseRegionIn *regs, size_t n_regions, PhaseRecord *out, PhasePileOut &pile) {
    using namespace phase_detail;
    std::vector<Region> regions(n_regions);
    for (size_t r = 0; r < n_regions; r++) {
        Region &lq = regions[r];
        lq.start = regs[r].start, lq.end = regs[r].end;
        lq.len = lq.n_cand = regs[r].n_cand;
        lq.indexs = 0;
        for (int c = 0; c < lq.n_cand; c++) lq.seqs[c] = Seq{regs[r].src[c], 0, regs[r].len[c], (uint8_t)c, regs[r].seq[c]};
        memset(&out[r], 0, sizeof(PhaseRecord));
    }
    pile = PhasePileOut();
    int s = 0, k = 0, j, index;
    std::vector<Phs> phase(n_aligned ? n_aligned : 1);
    int has_heter = 0;
    for (Region &lq : regions) {  // heterozygous sites first (:789-810)
        if (!lq.len) continue;
        select_most2(lq, lq.len, &s, &k);
        if (s != k && lq.seqs[k].kscore >= 3 && lq.seqs[s].len == lq.seqs[k].len) {
            if (s == 0 || k == 0) {
                const int heter = s == 0 ? k : s;
                for (j = 0; j < lq.len; j++) {
                    index = lq.seqs[j].order;
                    if (same_seq(lq.seqs[0], lq.seqs[j])) phase[index].s++;
                    else if (same_seq(lq.seqs[heter], lq.seqs[j])) phase[index].d++;
                }
            }
            lq.indexs = 1;
        } else lq.indexs = 0;
        if (!has_heter && (lq.indexs == 1 ||
                           (s != k && lq.seqs[k].kscore >= 5 && lq.seqs[s].kscore + lq.seqs[k].kscore >= lq.len * 0.8 &&
                            !prefixhomo_same(lq.seqs[s], lq.seqs[k]))))
            has_heter = 1;
    }
    pile.has_heter = (uint8_t)has_heter;
    if (has_heter && !phase[0].s) {  // :812-854
        pile.pass2 = 1;
        for (Region &lq : regions) {
            if (!lq.len) continue;
            select_most2_with_kscore(lq, lq.len, &s, &k);
            if (s != k && lq.seqs[k].kscore >= 5 && (lq.seqs[s].kscore + lq.seqs[k].kscore) >= lq.len * 0.8 &&
                (lq.seqs[s].len >= lq.seqs[k].len + 5 || lq.seqs[k].len >= lq.seqs[s].len + 5 || !prefixhomo_same(lq.seqs[s], lq.seqs[k]))) {
                int s_, k_;
                if (s == 0) { s_ = 1; k_ = 0; }
                else if (k == 0) { s_ = 0; k_ = 1; }
                else {
                    s_ = homo_end_same(lq.seqs[s], lq.seqs[0]) || trim_endssr_same(lq.seqs[s], lq.seqs[0]) ||
                         prefixhomo_same(lq.seqs[s], lq.seqs[0]);
                    k_ = homo_end_same(lq.seqs[k], lq.seqs[0]) || trim_endssr_same(lq.seqs[k], lq.seqs[0]) ||
                         prefixhomo_same(lq.seqs[k], lq.seqs[0]);
                }
                int same, heter;
                if (s_ && !k_) { same = s; heter = k; }
                else if (k_ && !s_) { same = k; heter = s; }
                else continue;
                for (j = 0; j < lq.len; j++) {
                    index = lq.seqs[j].order;
                    if (same_seq(lq.seqs[same], lq.seqs[j])) phase[index].s++;
                    else if (same_seq(lq.seqs[heter], lq.seqs[j])) phase[index].d++;
                }
                lq.indexs = 2;
            } else lq.indexs = 0;
        }
    }
    for (Region &lq : regions) {  // mark_del_lqseq, :570-588
        if (!lq.len) continue;
        int kk = 0;
        for (j = 1; j < lq.len; j++) {
            const int i = lq.seqs[j].order;
            if (phase[i].s >= 3 && !phase[i].d) kk++;
        }
        for (j = 0; j < lq.len; j++) {
            const int i = lq.seqs[j].order;
            if (kk >= 2) {
                if (phase[i].d) phase[i].del = 1;
            } else if (phase[i].s < phase[i].d || phase[i].d >= 3) phase[i].del = 1;
        }
    }
    for (Region &lq : regions) {  // remove_differ_phase_lqseq, :590-610
        if (!lq.len) continue;
        int8_t dif[kPhaseCanMax] = {0};
        for (j = 0; j < lq.len; j++)
            if (phase[lq.seqs[j].order].del) dif[j] = 1;
        compact_flagged(lq, dif);
    }
    std::vector<uint16_t> bins;
    std::vector<uint16_t> saved;
    for (size_t r = 0; r < n_regions; r++) {  // :874-984
        Region &lq = regions[r];
        PhaseRecord &o = out[r];
        if (!lq.n_cand) continue;   // (kPhaseEmpty)
        if (!lq.len) {              // every candidate's read was phased away
            write_record(lq, o, kPhaseDropped, 0);
            continue;
        }
        select_most2(lq, lq.len, &s, &k);
        index = lq.seqs[s].order;
        if (lq.indexs && s != k && s != 0 && lq.seqs[k].kscore >= 3 && phase[index].s >= phase[index].d + 3) {
            int sp = 0, kp = 0;
            for (j = 1; j < lq.len; j++) {
                index = lq.seqs[j].order;
                if (phase[index].d >= 3) continue;
                if (same_seq(lq.seqs[s], lq.seqs[j])) sp += phase[index].s - phase[index].d;
                else if (same_seq(lq.seqs[k], lq.seqs[j])) kp += phase[index].s - phase[index].d;
            }
            if (sp < kp) s = k;
        } else if (lq.seqs[0].len > 50 && lq.seqs[s].kscore < lq.len / 3 && lq.seqs[s].kscore < 3) {
            const int sl = remove_differ_len(lq);
            if (sl <= 3) {  // large length SD: keep the seed's own version
                s = 0;
                lq.seqs[s].kscore = 65534;
            }
        }
        if (lq.seqs[s].kscore > 2 || lq.seqs[s].kscore >= lq.len / 2) {
            o.lower = lq.seqs[s].kscore < lq.len / 2 ? 1 : 0;
            o.seed = lq.seqs[s].idx, o.seed_pos = (uint8_t)s;
            write_record(lq, o, kPhaseSeed, -2);
            continue;
        }
        remove_differ_len(lq);
        if (lq.len > 4) {
            std::stable_sort(lq.seqs, lq.seqs + lq.len, [](const Seq &a, const Seq &b) { return a.len < b.len; });  // compare_seq_by_len
            k = lq.len / 2;
            while (lq.len > k &&
                   (lq.seqs[lq.len - 1].len > 2 * lq.seqs[k].len || lq.seqs[lq.len - 1].len >= 1.4 * lq.seqs[lq.len - 2].len))
                lq.len--;
            if (k == lq.len) {
                write_record(lq, o, kPhaseDropped, 0);
                continue;
            }
            j = 0;
            k = lq.len / 2;
            if (lq.seqs[j].len < lq.seqs[k].len / 2) {
                std::reverse(lq.seqs, lq.seqs + lq.len);
                while (lq.seqs[lq.len - 1].len < lq.seqs[k].len / 2) lq.len--;
                if (k == lq.len) {
                    write_record(lq, o, kPhaseDropped, 0);
                    continue;
                }
            }
        }
        if (bins.empty()) bins.assign(65536, 0);
        rank_pass(lq, bins, 0);
        if (lq.seqs[0].len > 100) {
            o.tail = 1;
            saved.assign(n_aligned ? n_aligned : 1, 0);   // indexed by source read
            for (j = 0; j < lq.len; j++) saved[lq.seqs[j].order] = lq.seqs[j].kscore;
            rank_pass(lq, bins, 1);
            for (j = 0; j < lq.len; j++) lq.seqs[j].kscore = (uint16_t)(lq.seqs[j].kscore + saved[lq.seqs[j].order]);
        }
        // qsort(compare_seq_by_kscore): glibc's is a stable merge sort
        std::stable_sort(lq.seqs, lq.seqs + lq.len, [](const Seq &a, const Seq &b) { return a.kscore > b.kscore; });
        write_record(lq, o, kPhaseRanked, lq.len);
    }
}

}  // namespace ndgpu
