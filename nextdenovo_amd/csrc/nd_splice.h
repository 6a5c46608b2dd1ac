// The end of a pile: the splice of the regions' pseudo-seeds into the consensus (update_consensus_trimed), its table of lower-case
// runs (update_lqreg) and the clipping of terminal simple-sequence repeats (trim_terminal_ssr) -- lib/nextcorrect.c:1340-1482 and
// :2008-2128 -- stated once on the host: the engine (Impl::splice of consensus.cpp), the host flag of ndgpu_splice_batch and the tests
// share this statement; K24 (splice_kernel, msa_kernels.hip) is its device form.  Pure: no device, no environment.
// (Inline: a stand-alone sanitizer program of the tests includes this header and nothing else of the library.)
#pragma once

#include <cstdint>
#include <cstring>
#include <string>

namespace ndgpu {

constexpr int kSpliceLqRegMax = 10;   // LQREG_MAX_COUNT
constexpr uint32_t kSpliceMaxPos = (1u << 21) - 2u;   // the largest position a consensus word carries

struct SpliceLqReg {
    unsigned start = 0, end = 0, lqlen = 0, lq_total_len = 0;
};

// base_to_int (lib/nextcorrect.c:42-50): ACGT in either case 0 1 2 3 by the reference's order A T G C, N 5, M 6, anything else 4
struct SpliceBaseLut {      // (a table, not a switch: the bases are as good as random, and a branch per base is mispredicted)
    uint8_t v[256];
    constexpr SpliceBaseLut() : v() {
        for (int i = 0; i < 256; i++) v[i] = 4;
        v['A'] = v['a'] = 0;
        v['T'] = v['t'] = 1;
        v['G'] = v['g'] = 2;
        v['C'] = v['c'] = 3;
        v['N'] = 5;
        v['M'] = 6;
    }
};
inline constexpr SpliceBaseLut kSpliceBaseLut{};
inline uint8_t splice_base_code(unsigned char c) { return kSpliceBaseLut.v[c]; }

// :1340-1363, for the character at index p of seq
inline int splice_update_lqreg(SpliceLqReg *lq, const std::string &seq, unsigned p, int i, unsigned *hq_m, unsigned *lq_m) {
    if (seq[p] >= 'a') {
        if (!lq[i].lqlen) lq[i].start = p;
        if ((*lq_m)++ > 2) *hq_m = 0;
        lq[i].end = p;
        lq[i].lqlen++;
        lq[i].lq_total_len++;
    } else {
        if (lq[i].lqlen && lq[i].start == 0) {
            i++;
            *hq_m = 0;
        } else if (*hq_m + lq[i].start > lq[i].end || (*hq_m)++ > 10) {
            if (lq[i].end > lq[i].start + 100) i++;
            else lq[i].lqlen = lq[i].end = 0;
            *hq_m = 0;
        } else if (*hq_m >= lq[i].lqlen) {
            lq[i].lqlen = lq[i].end = 0;
            *hq_m = 0;
        }
        *lq_m = 0;
    }
    return i;
}

struct SpliceRegion {       // one region in the engine's order (the index counts down while the positions go up)
    uint32_t start = 0, end = 0;
    int32_t len = 0;        // usable when > 0 or == -2
    uint32_t sudoseed_len = 0;
    const char *sudoseed = nullptr;
};
inline bool splice_usable(int32_t len) { return len > 0 || len == -2; }

struct SpliceOut {
    std::string out;                        // the emitted string (cut where the tenth slot would open)
    SpliceLqReg lq[kSpliceLqRegMax + 1];    // the table as the loop left it; +1: the guard slot (the reference indexes lq[10] in one corner)
    int lq_i = 0;                           // after the `end == len - 1` bump
    uint32_t lq_m = 0, hq_m = 0;            // the chosen stretch [lq_m, hq_m) of `out`
    uint32_t lq_total_len = 0;              // in the reference's unsigned arithmetic
    uint32_t head_run = 0, tail_run = 0;    // HiFi: the lower-case runs at the two ends
    bool empty2 = false;                    // HiFi: nothing but lower case -- the len = 2 outcome
};

// :1365-1482 up to the result's length and identity.  words[i] = pos << 8 | char, i in [lstrip, len - rstrip) is read (anything
// indexable: an array of words, the engine's view of its consensus bases).
template <class Words>
inline void splice_host(const Words &words, uint32_t len, uint32_t lstrip, uint32_t rstrip, const SpliceRegion *regions, size_t n_regions,
                        bool hifi, SpliceOut &o) {
    o = SpliceOut();
    std::string &out = o.out;
    SpliceLqReg *lq = o.lq;
    unsigned p = 0, i = lstrip;
    int update = 1;
    int idx = (int)n_regions - 1;
    unsigned lq_m = 0, hq_m = 0;
    int lq_i = 0;
    auto usable = [&](int k) { return splice_usable(regions[k].len); };
    bool stop = false;
    while (!stop && i < len - rstrip) {
        p = words[i] >> 8;
        if (idx >= 0 && (!usable(idx) || p > regions[idx].end)) {
            idx--;
            update = 1;
        }
        if (idx >= 0 && usable(idx) && p >= regions[idx].start && p <= regions[idx].end) {
            if (update) {
                const SpliceRegion &r = regions[idx];
                for (unsigned j = 0; j < r.sudoseed_len; j++) {
                    out.push_back(r.sudoseed[j]);
                    lq_i = splice_update_lqreg(lq, out, (unsigned)out.size() - 1, lq_i, &hq_m, &lq_m);
                    if (lq_i >= kSpliceLqRegMax) { stop = true; break; }
                }
                update = 0;
            }
        } else {
            out.push_back((char)(words[i] & 0xffu));
            update = 1;
            lq_i = splice_update_lqreg(lq, out, (unsigned)out.size() - 1, lq_i, &hq_m, &lq_m);
            if (lq_i >= kSpliceLqRegMax) break;
        }
        i++;
    }
    const unsigned olen = (unsigned)out.size();
    if (lq_i < kSpliceLqRegMax + 1 && lq[lq_i].end == olen - 1) lq_i++;
    o.lq_i = lq_i;

    if (hifi) {
        unsigned a = 0, z = 0, lq_total_len = 0;
        while (a < olen && out[a] >= 'a') a++;
        while (z < olen && out[olen - 1 - z] >= 'a') z++;
        o.head_run = a, o.tail_run = z;
        if (a + z < olen) {
            for (int q = 0; q < lq_i && q < kSpliceLqRegMax + 1; q++) lq_total_len += lq[q].lq_total_len;
            o.lq_m = a, o.hq_m = olen - z;
            o.lq_total_len = lq_total_len - (a + z);
        } else {
            o.empty2 = true;
        }
        return;
    }
    if (lq_i) {
        lq_m = 0;
        hq_m = lq[0].start;
        p = lq[0].start;
        unsigned lq_total_len = lq[0].lq_total_len - lq[0].lqlen;
        for (i = 1; i < (unsigned)kSpliceLqRegMax && lq[i].end; i++) {
            if (lq[i].start - lq[i - 1].end > p) {
                lq_m = lq[i - 1].end + 1;
                hq_m = lq[i].start;
                lq_total_len = lq[i].lq_total_len - lq[i].lqlen;
                p = lq[i].start - lq[i - 1].end;
            }
        }
        if (i < (unsigned)kSpliceLqRegMax && olen - lq[i - 1].end > p) {
            lq_m = lq[i - 1].end + 1;
            hq_m = olen;
            lq_total_len = lq[i].lq_total_len;
        }
        o.lq_m = lq_m, o.hq_m = hq_m, o.lq_total_len = lq_total_len;
    } else {
        unsigned k = 0;
        while (k < olen && out[k] >= 'a') k++;
        o.head_run = k;
        o.lq_m = k, o.hq_m = olen;
        o.lq_total_len = lq[0].lq_total_len - k;
    }
}

// len and identity of the result before the trim (:1437-1439, :1470-1480) in the reference's arithmetic, whoever ran the loop
inline unsigned splice_len(uint32_t lq_m, uint32_t hq_m, bool empty2) { return empty2 ? 2u : hq_m - lq_m; }
inline float splice_identity(uint32_t lq_total_len, unsigned len, bool empty2) { return empty2 ? 0.0f : 1 - (float)lq_total_len / len; }
// the gate in front of trim_terminal_ssr (:1481): a float compared as a double
inline bool splice_trim_gate(unsigned len, float identity) { return len > 1000 && identity > 0.8; }

// ---- terminal SSR clipping (:2008-2128).  The 4-mer is a uint8_t shift-or of base_to_int: N (5) and M (6) carry a third bit into
// the low bit of the base before them, and lose it at the 4-mer's first base.
inline int splice_terminal_ssr(int *bins, int range, int klen, const char *seq, int s) {
    memset(bins, 0, sizeof(int) * 256);
    uint8_t km = 0;
    for (int i = 0; i < range; i++) {
        if (i) km = (uint8_t)(km << 2 | splice_base_code((unsigned char)seq[s + i + klen - 1]));
        else
            for (int k = 0; k < klen; k++) km = (uint8_t)(km << 2 | splice_base_code((unsigned char)seq[s + k]));
        bins[km]++;
    }
    int best = 0;
    for (int i = 0; i < 256; i++)
        if (bins[i] > best) {
            best = bins[i];
            km = (uint8_t)i;
        }
    return km;
}

inline int splice_clip_ssr(const char *seq, int seq_len, int klen, int kmer, int from_end) {
    const int gap = 20;
    int i, p = 0, p1 = 0, p2 = 0;
    uint8_t cur = 0;
    if (from_end) {
        uint8_t rk = 0;
        for (i = 0; i < 8; i += 2) rk = (uint8_t)(rk << 2 | (kmer >> i & 3));
        seq_len--;
        kmer = rk;
    }
    for (i = 0; i < seq_len - klen; i++) {
        if (from_end) {
            if (i) cur = (uint8_t)(cur << 2 | splice_base_code((unsigned char)seq[seq_len - i - klen + 1]));
            else
                for (int k = 0; k < klen; k++) cur = (uint8_t)(cur << 2 | splice_base_code((unsigned char)seq[seq_len - k]));
        } else {
            if (i) cur = (uint8_t)(cur << 2 | splice_base_code((unsigned char)seq[i + klen - 1]));
            else
                for (int k = 0; k < klen; k++) cur = (uint8_t)(cur << 2 | splice_base_code((unsigned char)seq[k]));
        }
        if (cur != kmer) {
            if (i - p > gap) {
                if (!p1) p1 = p;
                else if (p2) {
                    if (i - p2 < 100) { p = p1; break; }
                    else p1 = p2 = 0;
                }
            }
        } else {
            p = i;
            if (p1 && p2 == 0) p2 = p;
        }
    }
    return p > 100 ? p + klen : 0;
}

struct SsrTrim {
    int clip_s = 0, clip_e = 0;
    unsigned len = 0;       // the new length; 4: the clips leave 10 bases or fewer (the len = 4 outcome, the string stays as it was)
    bool ran = false;       // the gate let the trim run
};
// trim_terminal_ssr behind its gate: seq[0, len) with the identity splice_identity gave
inline SsrTrim ssr_trim_host(const char *seq, unsigned len, float identity) {
    SsrTrim t;
    t.len = len;
    if (!splice_trim_gate(len, identity)) return t;
    t.ran = true;
    int bins[256];
    const int range = 24, klen = 4;
    const int L = (int)len;
    int km = splice_terminal_ssr(bins, range, klen, seq, 0);
    if (bins[km] >= 4) {
        t.clip_s = splice_clip_ssr(seq, L, klen, km, 0);
        while (t.clip_s < L && seq[t.clip_s] >= 'a') t.clip_s++;
    }
    km = splice_terminal_ssr(bins, range, klen, seq, L - range - klen + 1);
    if (bins[km] >= 4) {
        t.clip_e = splice_clip_ssr(seq, L, klen, km, 1);
        while (t.clip_e < L && seq[L - t.clip_e - 1] >= 'a') t.clip_e++;
    }
    if (t.clip_s + t.clip_e < L - 10) t.len = (unsigned)(L - t.clip_s - t.clip_e);
    else t.len = 4;
    return t;
}

// One job's whole answer from the two statements above: what ndgpu_splice_batch reports and what the engine keeps.
struct SpliceAnswer {
    uint32_t len = 0;           // as the engine reports it, the codes 2 and 4 included
    uint32_t lq_total_len = 0;
    float identity = 0;
    uint32_t out_len = 0, lq_m = 0, hq_m = 0;
    int32_t lq_i = 0;
    int32_t clip_s = 0, clip_e = 0;
    uint32_t trimmed = 0;       // the gate let the trim run
    std::string seq;            // len bytes; len 2: empty; the len = 4 outcome of the trim: the first four bytes of the untrimmed stretch
};
// From the loop's integers (whoever ran it) and the stretch's first byte: length, identity and the trim.
inline void splice_finish(const char *stretch, uint32_t out_len, uint32_t lq_m, uint32_t hq_m, uint32_t lq_total_len, int lq_i, bool empty2,
                          SpliceAnswer &a) {
    a = SpliceAnswer();
    a.out_len = out_len, a.lq_m = lq_m, a.hq_m = hq_m, a.lq_i = lq_i, a.lq_total_len = lq_total_len;
    a.len = splice_len(lq_m, hq_m, empty2);
    a.identity = splice_identity(lq_total_len, a.len, empty2);
    if (empty2) return;
    const SsrTrim t = ssr_trim_host(stretch, a.len, a.identity);
    a.trimmed = t.ran ? 1u : 0u;
    a.clip_s = t.clip_s, a.clip_e = t.clip_e;
    if (t.ran && t.len == 4) {
        a.seq.assign(stretch, 4);
        a.len = 4;
    } else {
        a.seq.assign(stretch + t.clip_s, t.len);
        a.len = t.len;
    }
}
template <class Words>
inline void splice_answer_host(const Words &words, uint32_t len, uint32_t lstrip, uint32_t rstrip, const SpliceRegion *regions,
                               size_t n_regions, bool hifi, SpliceAnswer &a) {
    SpliceOut o;
    splice_host(words, len, lstrip, rstrip, regions, n_regions, hifi, o);
    splice_finish(o.out.c_str() + (o.empty2 ? 0 : o.lq_m), (uint32_t)o.out.size(), o.lq_m, o.hq_m, o.lq_total_len, o.lq_i, o.empty2, a);
}

}  // namespace ndgpu
