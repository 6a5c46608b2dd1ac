// Stand-alone check of cns_windows_host (csrc/nd_cns.h) for a sanitizer build: host code only, nothing preloaded.
// argv[1]: a file of int32 words -- n_cases, then per case: n, min_cov, lq_max_len, n x (t_pos, link, cov, base), the expected
// len, uncorrected_len, lstrip, rstrip, lqseq_total_length, n_regions, n_regions x (start, end), len x word.
// Exit status 0: every case equal; 1: a difference (printed); 2: the file could not be read.
#include <cstdio>
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
        const int n = next(), min_cov = next();
        const unsigned lq_max_len = (unsigned)next();
        std::vector<ndgpu::PathStep> steps((size_t)n);
        for (int k = 0; k < n; k++) {
            steps[k].t_pos = next();
            steps[k].link = (uint16_t)next();
            steps[k].cov = (uint16_t)next();
            steps[k].base = (uint8_t)next();
            steps[k].delta = 0;
        }
        std::vector<uint32_t> words;
        std::vector<ndgpu::CnsWindow> wins;
        ndgpu::CnsCounts cnt;
        ndgpu::cns_windows_host(steps.data(), steps.size(), min_cov, lq_max_len, words, wins, cnt);
        const uint32_t got[5] = {cnt.len, cnt.uncorrected_len, cnt.lstrip, cnt.rstrip, cnt.lqseq_total_length};
        bool same = true;
        for (int k = 0; k < 5; k++) same = ((uint32_t)next() == got[k]) && same;
        const uint32_t n_reg = (uint32_t)next();
        same = same && n_reg == wins.size();
        for (uint32_t k = 0; k < n_reg; k++) {
            const uint32_t s = (uint32_t)next(), e = (uint32_t)next();
            same = same && k < wins.size() && wins[k].start == s && wins[k].end == e;
        }
        for (uint32_t k = 0; k < got[0]; k++) same = ((uint32_t)next() == words[k]) && same;
        if (!same) {
            fprintf(stderr, "case %d differs\n", c);
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
