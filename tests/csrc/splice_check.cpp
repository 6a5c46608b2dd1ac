// Stand-alone check of the host statement of the splice, its table of lower-case runs and the SSR trim (csrc/nd_splice.h), built with
// -fsanitize=address,undefined by tests/test_simt_splice.py.  Reads a file of int32 words: the number of jobs, then per job
//   n_words, lstrip, rstrip, read_type, n_regions, the words, per region start, end, len, sudoseed_len and its bytes (one a word),
//   and what the Python restatement expects: len, lq_total_len, the identity's bits (-1: a NaN), out_len, lq_m, hq_m, lq_i, clip_s,
//   clip_e, seq_len and the result's bytes, the 44 words of the table (ten slots and the guard slot: start, end, lqlen,
//   lq_total_len), and the out_len emitted characters.
// Every region's pseudo-seed and every word array lives in a heap block of its exact size, so that a read past either is seen.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "nd_splice.h"

using namespace ndgpu;

int main(int argc, char **argv) {
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "rb");
    if (!f) return 2;
    std::vector<int32_t> w;
    int32_t buf[4096];
    size_t got;
    while ((got = fread(buf, sizeof(int32_t), 4096, f)) > 0) w.insert(w.end(), buf, buf + got);
    fclose(f);
    size_t at = 0;
    auto next = [&]() { return w.at(at++); };
    const int n = next();
    int bad = 0;
    for (int c = 0; c < n; c++) {
        const uint32_t n_words = (uint32_t)next(), lstrip = (uint32_t)next(), rstrip = (uint32_t)next();
        const int read_type = next();
        const size_t n_regions = (size_t)next();
        std::unique_ptr<uint32_t[]> words(new uint32_t[n_words]);
        for (uint32_t k = 0; k < n_words; k++) words[k] = (uint32_t)next();
        std::vector<SpliceRegion> regions(n_regions);
        std::vector<std::unique_ptr<char[]>> seeds(n_regions);
        for (size_t k = 0; k < n_regions; k++) {
            SpliceRegion &r = regions[k];
            r.start = (uint32_t)next(), r.end = (uint32_t)next(), r.len = next(), r.sudoseed_len = (uint32_t)next();
            seeds[k].reset(new char[r.sudoseed_len]);
            for (uint32_t j = 0; j < r.sudoseed_len; j++) seeds[k][j] = (char)next();
            r.sudoseed = seeds[k].get();
        }
        const uint32_t e_len = (uint32_t)next(), e_total = (uint32_t)next();
        const int32_t e_bits = next();
        const uint32_t e_out_len = (uint32_t)next(), e_lq_m = (uint32_t)next(), e_hq_m = (uint32_t)next();
        const int e_lq_i = next(), e_clip_s = next(), e_clip_e = next();
        std::string e_seq((size_t)next(), '\0');
        for (char &ch : e_seq) ch = (char)next();
        uint32_t e_tab[44];
        for (uint32_t &v : e_tab) v = (uint32_t)next();
        std::string e_out(e_out_len, '\0');
        for (char &ch : e_out) ch = (char)next();

        SpliceOut o;
        splice_host(words.get(), n_words, lstrip, rstrip, regions.data(), n_regions, read_type == 3, o);
        SpliceAnswer a;
        splice_answer_host(words.get(), n_words, lstrip, rstrip, regions.data(), n_regions, read_type == 3, a);
        int32_t bits;
        memcpy(&bits, &a.identity, 4);
        if (a.identity != a.identity) bits = -1;
        bool ok = a.len == e_len && a.lq_total_len == e_total && bits == e_bits && a.out_len == e_out_len && a.lq_m == e_lq_m &&
                  a.hq_m == e_hq_m && a.lq_i == e_lq_i && a.clip_s == e_clip_s && a.clip_e == e_clip_e && a.seq == e_seq && o.out == e_out;
        for (int s = 0; s < 11; s++)
            ok = ok && o.lq[s].start == e_tab[4 * s] && o.lq[s].end == e_tab[4 * s + 1] && o.lq[s].lqlen == e_tab[4 * s + 2] &&
                 o.lq[s].lq_total_len == e_tab[4 * s + 3];
        if (!ok) {
            printf("case %d differs: len %u/%u total %u/%u bits %d/%d out_len %u/%u stretch [%u, %u)/[%u, %u) lq_i %d/%d clips %d %d/%d %d\n", c,
                   a.len, e_len, a.lq_total_len, e_total, bits, e_bits, a.out_len, e_out_len, a.lq_m, a.hq_m, e_lq_m, e_hq_m, a.lq_i, e_lq_i,
                   a.clip_s, a.clip_e, e_clip_s, e_clip_e);
            bad++;
        }
    }
    if (at != w.size()) {
        printf("trailing words\n");
        return 1;
    }
    if (bad) return 1;
    printf("%d cases checked\n", n);
    return 0;
}
