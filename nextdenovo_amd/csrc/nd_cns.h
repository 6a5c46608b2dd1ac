// The consensus bases and low-quality windows of the main walk (generate_cns_from_best_score's loop, lib/nextcorrect.c:1907-1982),
// stated once on the host: the engine (Impl::cns_from_best_score of consensus.cpp), the host flag of ndgpu_cns_windows_batch and the
// tests share this statement; K20 (cns_windows_kernel, msa_kernels.hip) is its device form.  Pure: no device, no environment.
// (Inline: a stand-alone sanitizer program of the tests includes this header and nd_host.h and nothing else.)
#pragma once

#include <cctype>
#include <cstdint>
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

}  // namespace ndgpu
