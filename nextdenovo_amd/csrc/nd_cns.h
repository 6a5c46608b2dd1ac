// The consensus bases and low-quality windows of the main walk (generate_cns_from_best_score's loop, lib/nextcorrect.c:1907-1982),
// stated once on the host: the engine (Impl::cns_from_best_score of consensus.cpp), the host flag of ndgpu_cns_windows_batch and the
// tests share this statement; K20 (cns_windows_kernel, msa_kernels.hip) is its device form.  Pure: no device, no environment.
// (Inline: a stand-alone sanitizer program of the tests includes this header and nd_host.h and nothing else.)
#pragma once

#include <algorithm>
#include <cctype>
#include <cstdint>
#include <string>
#include <vector>

#include "nd_host.h"

namespace ndgpu {

struct CnsWindow {          // one low-quality window in seed positions, as the reference's lqseq: start belongs to the later index
    uint32_t start, end;
};
struct CnsCounts {
    uint32_t len = 0;                 // consensus bases (non-gap steps), lstrip and rstrip included
    uint32_t uncorrected_len = 0;     // lower-case bases
    uint32_t lstrip = 0;              // the lower-case run at the walk's end
    uint32_t rstrip = 0;              // the lower-case run at its start
    uint32_t lqseq_total_length = 0;  // bases with pqv <= 40
};
constexpr unsigned char kCnsIntToBase[8] = {'A', 'T', 'G', 'C', '-', 'N', 'M', 'M'};  // int_to_base (lib/nextcorrect.c:52-62)

// steps: the walk, origin first; a non-gap step needs cov > 0.  words[p] = pos << 8 | char for the p-th non-gap step, as the
// reference numbers them before reverse_consensus_base; wins in emission order.  The verdict (len > 2, the 0.8 test, the ratio test)
// and the reversal stay with the caller.
inline void cns_windows_host(const PathStep *steps, size_t n, int min_cov, unsigned lq_max_len, std::vector<uint32_t> &words,
                             std::vector<CnsWindow> &wins, CnsCounts &c) {
    int p = 0, lable = 1;
    const int lq_min_length = 8;
    int qv = 0, pqv, hq = 0, lq = 0, lq_l = 0, lq_s = -1, lq_e = -1;
    c = CnsCounts();
    words.clear();
    wins.clear();
    words.reserve(n);
    auto pos_at = [&](int i) { return words[(size_t)i] >> 8; };
    for (size_t k = 0; k < n; k++) {
        const PathStep &cur = steps[k];
        if (cur.base == 4) continue;
        const uint32_t pos = (uint32_t)cur.t_pos;
        words.push_back(pos << 8);
        const int cov = cur.cov;
        pqv = 100 * (int)cur.link / cov;
        if (pqv > 40) hq++;
        else {
            hq = 0;
            c.lqseq_total_length++;
        }
        if (hq > lq_min_length / 2 && lq_e - lq_s < lq_min_length / 2) {
            qv = lq_l = lq = 0;
            lq_s = -1;
        }
        if ((qv + pqv) / (lq_l + 1) < 40) {
            if (lq_s == -1) lq_s = p;
            lq_e = p;
            lq = 1;
            lq_l++;
            qv += pqv;
        } else if (lq && p - lq_e > 2 * lq_min_length && pos_at(p) != pos_at(p - 1)) {
            if (lq_e - lq_s + 1 > lq_min_length && (unsigned)(lq_e - lq_s + 1) < lq_max_len) {
                lq_e = p - lq_min_length - 1;
                lq_s = lq_s > lq_min_length ? lq_s - lq_min_length : 1;
                CnsWindow r;
                r.end = pos_at(lq_s);
                r.start = pos_at(lq_e);
                if (!wins.empty() && r.end == wins.back().start) {
                    while (r.end == wins.back().start && lq_s < p - 4) r.end = pos_at(++lq_s);
                }
                wins.push_back(r);
            }
            qv = lq_l = lq = 0;
            lq_s = -1;
        } else if (lq && pos_at(p) != pos_at(p - 1)) {
            qv = lq_l = 0;
        }
        if (cov > min_cov && pqv > 20) {
            words[(size_t)p] |= kCnsIntToBase[cur.base & 7];
            lable = 0;
            c.lstrip = 0;
        } else {
            words[(size_t)p] |= (unsigned char)tolower(kCnsIntToBase[cur.base & 7]);
            c.uncorrected_len++;
            c.lstrip++;
            if (lable) c.rstrip++;
        }
        p++;
    }
    c.len = (uint32_t)p;
}

// The verdict of generate_cns_from_best_score (lib/nextcorrect.c:1986-1987) in the reference's unsigned / float / double arithmetic.
inline bool cns_verdict(const CnsCounts &c, float min_error_corrected_ratio) {
    const float lhs = (float)(c.uncorrected_len - c.lstrip - c.rstrip);
    const float rhs = (float)(c.len - c.lstrip - c.rstrip) * (1 - min_error_corrected_ratio);
    return c.len > 2 && (double)(int)c.lqseq_total_length < c.len * 0.8 && lhs < rhs;
}

// ---- the two other forms of "after main": HiFi reads (generate_cns_from_best_score_kmer, lib/nextcorrect.c:1786-1883) and -fast
// (generate_cns_from_best_score_fast, :1717-1784).  The engine (Impl::cns_kmer, Impl::cns_fast of consensus.cpp), the host flag of
// ndgpu_cns_walk_batch and the tests share these statements; K21 (cns_walk_kernel, msa_kernels.hip) is their device form.

// base_to_int for a seed's byte (lib/nextcorrect.c:42-50): what the engine's table gives
struct CnsBaseLut {         // (a table, not a switch: the bases are as good as random, and a branch per item is mispredicted)
    uint8_t v[256];
    constexpr CnsBaseLut() : v() {
        for (int i = 0; i < 256; i++) v[i] = 4;
        v['A'] = v['a'] = 0;
        v['T'] = v['t'] = 1;
        v['G'] = v['g'] = 2;
        v['C'] = v['c'] = 3;
        v['N'] = 5;
        v['M'] = 6;
    }
};
inline constexpr CnsBaseLut kCnsBaseLut{};
inline uint8_t cns_base_code(unsigned char c) { return kCnsBaseLut.v[c]; }
struct CnsSeedAscii {       // a seed's codes read off its ASCII bytes
    const char *s;
    uint8_t operator[](size_t t) const { return cns_base_code((unsigned char)s[t]); }
};

// The loop of :1807-1860.  seed_codes[t]: the seed's code at position t (anything indexable: a code array, CnsSeedAscii); every
// non-gap step needs cov > 0 and a t_pos inside the seed.  words / wins as cns_windows_host gives them (wins in push order, a merge
// rewrites the last one's start); c.len and c.lqseq_total_length are counted, the other three counters stay 0 in this variant.
template <class Seed>
inline void cns_kmer_host(const PathStep *steps, size_t n, const Seed &seed_codes, int min_cov, std::vector<uint32_t> &words,
                          std::vector<CnsWindow> &wins, CnsCounts &c) {
    const int lq_min_length = 2, dag_min_qv = 80;
    int p = 0, qv, lq = 0, lq_s = -1, lq_e = -1;
    c = CnsCounts();
    words.clear();
    wins.clear();
    words.reserve(n);
    auto pos_at = [&](int i) { return words[(size_t)i] >> 8; };
    for (size_t k = 0; k < n; k++) {
        const PathStep &cur = steps[k];
        if (cur.base == 4) continue;
        words.push_back((uint32_t)cur.t_pos << 8);
        const int cov = cur.cov;
        qv = 100 * (int)cur.link / cov;
        if (cov < 4) {
            lq = 0;
            lq_s = -1;
            c.lqseq_total_length++;
        } else if (qv < dag_min_qv || cur.base != seed_codes[(size_t)cur.t_pos]) {
            if (lq_s == -1) lq_s = p;
            lq_e = p;
            lq = 1;
            c.lqseq_total_length++;
        } else if (lq && p - lq_e > 2 * lq_min_length && pos_at(p) != pos_at(p - 1)) {
            lq_e = p - lq_min_length - 1;
            lq_s = lq_s > lq_min_length ? lq_s - lq_min_length : 1;
            if (!wins.empty() && pos_at(lq_s) >= wins.back().start) {
                wins.back().start = pos_at(lq_e);
            } else {
                CnsWindow r;
                r.end = pos_at(lq_s);
                r.start = pos_at(lq_e);
                wins.push_back(r);
            }
            lq = 0;
            lq_s = -1;
        }
        const unsigned char ch = kCnsIntToBase[cur.base & 7];
        words[(size_t)p] |= cov > min_cov ? ch : (unsigned char)tolower(ch);
        p++;
    }
    c.len = (uint32_t)p;
}

// The verdict of generate_cns_from_best_score_kmer (:1864-1865): uncorrected_len, lstrip and rstrip are 0 there.
inline bool cns_kmer_verdict(const CnsCounts &c, float min_error_corrected_ratio) {
    const float rhs = (float)c.len * (1 - min_error_corrected_ratio);
    return c.len > 2 && (double)(int)c.lqseq_total_length < c.len * 0.8 && 0.0f < rhs;
}

constexpr int kCnsLqRegMax = 10;  // LQREG_MAX_COUNT
struct CnsFastOut {
    uint32_t lq_m = 0, hq_m = 0;   // the chosen stretch [lq_m, hq_m) of the emitted string
    uint32_t lq_total_len = 0;
    uint32_t out_len = 0;          // characters emitted (the walk is cut where the tenth slot would open)
    std::string seq;               // the stretch, reversed
};
// :1724-1777: the emitted string with its table of kCnsLqRegMax lower-case runs (slot 0 closes at the first upper-case character
// whatever its length, a later one at end >= start + 50; end == 0 means "empty", so a run at index 0 opens again at index 1), the
// scan over the table for the longest stretch between closed runs, and the tail behind the last one.
inline void cns_fast_host(const PathStep *steps, size_t n, int min_cov, CnsFastOut &o) {
    struct Reg { unsigned start = 0, end = 0, lqlen = 0, lq_total_len = 0; };
    std::string out;
    Reg lq[kCnsLqRegMax];
    int lq_i = 0;
    for (size_t k = 0; k < n; k++) {
        const PathStep &cur = steps[k];
        if (cur.base != 4) {
            if ((int)cur.cov > min_cov) {
                out.push_back((char)kCnsIntToBase[cur.base & 7]);
                if (lq[lq_i].end >= lq[lq_i].start + 50 || !lq_i) {
                    if (++lq_i >= kCnsLqRegMax) break;
                } else lq[lq_i].end = 0;
            } else {
                out.push_back((char)tolower(kCnsIntToBase[cur.base & 7]));
                if (!lq[lq_i].end) {
                    lq[lq_i].start = (unsigned)out.size() - 1;
                    lq[lq_i].lqlen = 0;
                }
                lq[lq_i].end = (unsigned)out.size() - 1;
                lq[lq_i].lq_total_len++;
                lq[lq_i].lqlen++;
            }
        }
    }
    int i, lq_m = 0, hq_m = (int)lq[0].start, l = hq_m;
    unsigned lq_total_len = lq[0].lq_total_len - lq[0].lqlen;
    for (i = 1; i < kCnsLqRegMax && lq[i].end; i++) {
        if (lq[i].start - lq[i - 1].end > (unsigned)l) {
            lq_m = (int)lq[i - 1].end + 1;
            hq_m = (int)lq[i].start;
            lq_total_len = lq[i].lq_total_len - lq[i].lqlen;
            l = hq_m - lq_m;
        }
    }
    if (i < kCnsLqRegMax && (unsigned)out.size() - lq[i - 1].end > (unsigned)l) {
        lq_m = (int)lq[i - 1].end + 1;
        hq_m = (int)out.size();
        lq_total_len = lq[i].lq_total_len;
    }
    o.lq_m = (uint32_t)lq_m, o.hq_m = (uint32_t)hq_m, o.lq_total_len = lq_total_len, o.out_len = (uint32_t)out.size();
    o.seq = (size_t)lq_m <= out.size() ? out.substr((size_t)lq_m, (unsigned)(hq_m - lq_m)) : std::string();
    std::reverse(o.seq.begin(), o.seq.end());
}
// len and identity of the -fast result (:1778-1779) in the reference's arithmetic, whoever ran the loop
inline unsigned cns_fast_len(uint32_t lq_m, uint32_t hq_m) { return (unsigned)((int)hq_m - (int)lq_m); }
inline float cns_fast_identity(uint32_t lq_total_len, unsigned len) { return 1 - (float)lq_total_len / len; }

}  // namespace ndgpu
