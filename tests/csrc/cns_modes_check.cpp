// Stand-alone check of cns_kmer_host and cns_fast_host (csrc/nd_cns.h) for a sanitizer build: host code only, nothing preloaded.
// argv[1]: a file of int32 words -- n_cases, then per case: mode, n, min_cov, n x (t_pos, link, cov, base), and
//   mode 1: seed_len, seed_len x byte, the expected len, lqseq_total_length, n_regions, n_regions x (start, end), len x word;
//   mode 2: the expected len (hq_m - lq_m), lq_total_len, characters emitted, seq_len, seq_len x byte.
// Exit status 0: every case equal; 1: a difference (printed); 2: the file could not be read.
#include <cstdio>
#include <string>
#include <vector>

#include "nd_cns.h"

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> w;
    int32_t buf[4096];
    for (size_t k; (k = fread(buf, sizeof(int32_t), 4096, f)) > 0;) w.insert(w.end(), buf, buf + k);
    fclose(f);
    size_t at = 0;
    auto next = [&]() -> int32_t { return at < w.size() ? w[at++] : (at++, 0); };
    const int n_cases = next();
    int bad = 0;
    for (int c = 0; c < n_cases; c++) {
        const int mode = next(), n = next(), min_cov = next();
        std::vector<ndgpu::PathStep> steps((size_t)n);
        for (int k = 0; k < n; k++) {
            steps[k].t_pos = next();
            steps[k].link = (uint16_t)next();
            steps[k].cov = (uint16_t)next();
            steps[k].base = (uint8_t)next();
            steps[k].delta = 0;
        }
        bool same = true;
        if (mode == 1) {
            const int seed_len = next();
            std::string seed((size_t)seed_len, 'A');   // (exact size: a read past the seed is the sanitizer's to find)
            for (int k = 0; k < seed_len; k++) seed[(size_t)k] = (char)next();
            std::vector<uint8_t> codes((size_t)seed_len);
            for (int k = 0; k < seed_len; k++) codes[(size_t)k] = ndgpu::cns_base_code((unsigned char)seed[(size_t)k]);
            std::vector<uint32_t> words, words2;
            std::vector<ndgpu::CnsWindow> wins, wins2;
            ndgpu::CnsCounts cnt, cnt2;
            ndgpu::cns_kmer_host(steps.data(), steps.size(), ndgpu::CnsSeedAscii{seed.data()}, min_cov, words, wins, cnt);
            ndgpu::cns_kmer_host(steps.data(), steps.size(), codes.data(), min_cov, words2, wins2, cnt2);   // the batched entry's form
            same = words == words2 && wins.size() == wins2.size() && cnt.len == cnt2.len && cnt.lqseq_total_length == cnt2.lqseq_total_length;
            same = ((uint32_t)next() == cnt.len) && same;
            same = ((uint32_t)next() == cnt.lqseq_total_length) && same;
            same = same && cnt.uncorrected_len == 0 && cnt.lstrip == 0 && cnt.rstrip == 0;
            const uint32_t n_reg = (uint32_t)next();
            same = same && n_reg == wins.size();
            for (uint32_t k = 0; k < n_reg; k++) {
                const uint32_t s = (uint32_t)next(), e = (uint32_t)next();
                same = same && k < wins.size() && wins[k].start == s && wins[k].end == e && wins2[k].start == s && wins2[k].end == e;
            }
            for (uint32_t k = 0; k < cnt.len; k++) same = ((uint32_t)next() == words[k]) && same;
        } else {
            ndgpu::CnsFastOut o;
            ndgpu::cns_fast_host(steps.data(), steps.size(), min_cov, o);
            same = ((uint32_t)next() == ndgpu::cns_fast_len(o.lq_m, o.hq_m)) && same;
            same = ((uint32_t)next() == o.lq_total_len) && same;
            same = ((uint32_t)next() == o.out_len) && same;
            const uint32_t seq_len = (uint32_t)next();
            same = same && seq_len == o.seq.size();
            for (uint32_t k = 0; k < seq_len; k++) {
                const char ch = (char)next();
                same = same && k < o.seq.size() && o.seq[k] == ch;
            }
        }
        if (!same) {
            fprintf(stderr, "case %d (mode %d) differs\n", c, mode);
            bad = 1;
        }
    }
    if (at != w.size()) {
        fprintf(stderr, "file length: read %zu of %zu words\n", at, w.size());
        bad = 1;
    }
    printf("%d cases checked\n", n_cases);
    return bad;
}
