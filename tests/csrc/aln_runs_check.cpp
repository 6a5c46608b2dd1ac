// TEST INFRASTRUCTURE ONLY.  A stand-alone program around aln_runs_host (csrc/nd_host.h), the host form of K15 that the batched
// alignment entry's host flag reports from: built with -fsanitize=address,undefined by tests/test_simt_align_batch.py and fed column
// streams on stdin -- per stream a uint32 count and that many bytes (0 match, 1 query only, 2 target only).  Prints per stream
// "n_runs n_match n_ins n_del max_gap_run aln_len" and the runs; streams are copied into exact-size heap blocks so that a read past
// either end is an error, not a neighbour's byte.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "nd_host.h"

int main() {
    uint32_t n = 0;
    std::vector<uint32_t> runs;
    while (fread(&n, sizeof(n), 1, stdin) == 1) {
        uint8_t *ops = new uint8_t[n ? n : 1];
        if (n && fread(ops, 1, n, stdin) != n) return 2;
        ndgpu::AlnRunsResult r;
        const size_t before = runs.size();
        ndgpu::aln_runs_host(ops, n, r, runs);
        delete[] ops;
        if (r.run_off != before || runs.size() - before != r.n_runs) return 3;
        printf("%u %u %u %u %u %u", r.n_runs, r.n_match, r.n_ins, r.n_del, r.max_gap_run, r.aln_len);
        for (size_t k = before; k < runs.size(); k++) printf(" %u", runs[k]);
        printf("\n");
    }
    return 0;
}
