// How a batch call's length-sorted piles are cut into sub-batches (ndgpu_correct_piles_stream): pure arithmetic, no device, no
// environment -- a plain C++ program can include this header and nothing else (tests/csrc/sub_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <vector>

namespace ndgpu {

// The share of the call's cost each round of the contexts takes.  Default: per_ctx equal rounds.  spec (NDGPU_TAPER=w1,w2,...)
// replaces them by its positive numbers, normalised; a spec without one leaves the default.  Rounds may taper because of what the
// LAST round leaves for the host -- its piles' candidate ranking, POA, two more rounds -- ends the call with the device idle, and it
// is that round's share of the call's host work divided by the CPUs the process has.
inline std::vector<double> round_weights(int per_ctx, const char *spec) {
    std::vector<double> weights((size_t)per_ctx, 1.0 / per_ctx);
    if (!spec) return weights;
    std::vector<double> w;
    for (const char *p = spec; *p;) {
        char *end = nullptr;
        const double v = strtod(p, &end);
        if (end == p) break;
        if (v > 0) w.push_back(v);
        p = *end ? end + 1 : end;
    }
    double sum = 0;
    for (double v : w) sum += v;
    if (!w.empty() && sum > 0) {
        for (double &v : w) v /= sum;
        weights = w;
    }
    return weights;
}

// Sub-batches = consecutive ranges of the length-sorted piles of (about) equal cost, weights.size() per context, pulled from one
// queue by whichever context is free.  est[k] = the cost of pile k: estimated alignment columns (what every device phase and the
// host's low-quality-region stage scale with).  A context alternates device-heavy phases (alignment, MSA, scoring) with host-heavy
// ones (candidate ranking, POA, second MSA, splicing): with several sub-batches per context the phases of different contexts
// interleave instead of all contexts being on the host -- and the device idle -- at the end of a call.  (Until round 2 the first
// sub-batches were small and held the longest seeds, because a seed's scoring chain bounded the call; the segment-parallel scoring
// DP removed that.)
// (Measured on config 2, 1,666 piles: 1, 2, 3, 4, 6 per context = 1147, 1095, 1181, 1269, 1376 ms per step in round 2; 1 and 2
// within noise since.  A small call -- the share of one rank of 4 or 8 -- is a matter of latency, not of filling the device: every
// sub-batch of a context is another pass through the same dependent phases, and with one per context the 210 piles of a rank of 8
// take 170 ms instead of 262, the 407 of a rank of 4 255 instead of 320: profiles/r04_rank_share_config2.txt)
//
// Exactly drivers x weights.size() pieces of equal cost where the caps allow it (a cut where the running cost passes the next
// multiple of total / pieces): with "cut before the piece would overflow" the pieces came out slightly small and a 17th, alone in a
// third round of the contexts, ended every config-2 call ~60 ms late.  The caps still cut: at most max_piles piles and at most
// tag_budget columns a piece (a pile on its own may exceed it), so that the device buffers of a context -- sized by the largest
// sub-batch it has seen -- stay bounded whatever the seed lengths.
// Returns the cuts: piece j is piles [cuts[j], cuts[j + 1]); cuts.front() == 0, cuts.back() == est.size().
inline std::vector<size_t> plan_sub_batches(const std::vector<uint64_t> &est, int drivers, const std::vector<double> &weights,
                                            size_t max_piles, uint64_t tag_budget) {
    uint64_t total = 0;
    for (uint64_t e : est) total += e;
    std::vector<uint64_t> targets;   // cumulative cost at which piece k ends
    double at = 0;
    for (double w : weights)
        for (int c = 0; c < drivers; c++) {
            at += w / drivers;
            targets.push_back((uint64_t)(at * (double)total));
        }
    if (!targets.empty()) targets.pop_back();  // (the last piece ends with the piles)
    const uint64_t n_target = (uint64_t)targets.size() + 1;
    const uint64_t piece = std::min<uint64_t>(tag_budget, std::max<uint64_t>(total / n_target + 1, 2000000ull));
    const bool by_target = total / n_target + 1 <= tag_budget && total / n_target + 1 >= 2000000ull;  // (neither cap nor floor bites)
    std::vector<size_t> cuts{0};
    uint64_t acc = 0, run = 0;
    size_t cnt = 0, next_cut = 0;
    for (size_t k = 0; k < est.size(); k++) {
        bool cut = cnt && (cnt >= max_piles || acc + est[k] > tag_budget);
        if (!cut && cnt) {
            if (by_target) cut = next_cut < targets.size() && run + est[k] / 2 >= targets[next_cut];
            else cut = acc + est[k] > piece;
        }
        if (cut) {
            cuts.push_back(k);
            acc = 0, cnt = 0;
            while (by_target && next_cut < targets.size() && run + est[k] / 2 >= targets[next_cut]) next_cut++;
        }
        acc += est[k], run += est[k], cnt++;
    }
    cuts.push_back(est.size());
    return cuts;
}

}  // namespace ndgpu
