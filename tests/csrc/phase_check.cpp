// Stand-alone check of hifi_phase_host (csrc/nd_phase.h) for a sanitizer build: host code only, nothing preloaded.
// argv[1]: a file of int32 words -- n_piles, then per pile: n_aligned, n_regions, has_heter, pass2, and per region: start, end, n_cand,
//   n_cand x (source read, len, len x byte), then the expected record: kind, lower, indexs, tail, n, seed, seed_pos, n_cand x perm,
//   n_cand x kscore.
// Exit status 0: every pile equal; 1: a difference (printed); 2: the file could not be read.
#include <cstdio>
#include <string>
#include <vector>

#include "nd_phase.h"

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
    const int n_piles = next();
    int bad = 0;
    for (int p = 0; p < n_piles; p++) {
        const unsigned n_aligned = (unsigned)next();
        const int n_regions = next(), has_heter = next(), pass2 = next();
        std::vector<ndgpu::PhaseRegionIn> in((size_t)n_regions);
        std::vector<ndgpu::PhaseRecord> want((size_t)n_regions), got((size_t)n_regions);
        // every candidate in a heap block of its exact size: a read past it is the sanitizer's to find
        std::vector<std::vector<std::vector<char>>> bytes((size_t)n_regions);
        std::vector<std::vector<const char *>> ptr((size_t)n_regions);
        std::vector<std::vector<uint16_t>> len((size_t)n_regions), src((size_t)n_regions);
        for (int r = 0; r < n_regions; r++) {
            const uint32_t start = (uint32_t)next(), end = (uint32_t)next();
            const int nc = next();
            bytes[r].resize((size_t)nc), ptr[r].resize((size_t)nc), len[r].resize((size_t)nc), src[r].resize((size_t)nc);
            for (int c = 0; c < nc; c++) {
                src[r][c] = (uint16_t)next();
                len[r][c] = (uint16_t)next();
                bytes[r][c].resize(len[r][c]);
                for (int b = 0; b < len[r][c]; b++) bytes[r][c][(size_t)b] = (char)next();
                ptr[r][c] = bytes[r][c].data();
            }
            in[r] = ndgpu::PhaseRegionIn{start, end, nc, ptr[r].data(), len[r].data(), src[r].data()};
            ndgpu::PhaseRecord &o = want[r];
            memset(&o, 0, sizeof(o));
            o.kind = (uint8_t)next(), o.lower = (uint8_t)next(), o.indexs = (uint8_t)next(), o.tail = (uint8_t)next();
            o.n = (int16_t)next(), o.seed = (uint8_t)next(), o.seed_pos = (uint8_t)next();
            for (int c = 0; c < nc; c++) o.perm[c] = (uint8_t)next();
            for (int c = 0; c < nc; c++) o.kscore[c] = (uint16_t)next();
        }
        ndgpu::PhasePileOut pile;
        ndgpu::hifi_phase_host(n_aligned, in.data(), in.size(), got.data(), pile);
        bool same = pile.has_heter == has_heter && pile.pass2 == pass2;
        for (int r = 0; r < n_regions; r++) same = same && memcmp(&want[r], &got[r], sizeof(ndgpu::PhaseRecord)) == 0;
        if (!same) {
            fprintf(stderr, "pile %d differs\n", p);
            bad = 1;
        }
    }
    if (at != w.size()) {
        fprintf(stderr, "file length: read %zu of %zu words\n", at, w.size());
        bad = 1;
    }
    printf("%d piles checked\n", n_piles);
    return bad;
}
