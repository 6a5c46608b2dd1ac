// The two planners of the phases behind the main phase (device_runtime.hip): how a low-quality-region round is cut into K12a's jobs
// (run_lq) and how a POA round is cut into launches by the cell budget (run_poa).  Pure arithmetic, no device, no environment -- a
// plain C++ program can include this header and nothing else (tests/csrc/lq_plan_check.cpp).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace ndgpu {

struct LqRegionLoad {     // one region of a round, over its rows (30: nd_device.h, kLqRoundRows)
    uint32_t sl;          // columns of the region's pseudo-seed
    uint64_t q_bases;     // sum of q_len over the rows that have a job
    uint64_t qt_bases;    // sum of q_len + t_len over the same rows
    uint32_t empty_rows;  // rows without a job
};
struct LqJobCut {         // regions [g_a, g_b) = columns [t0, t1) of the linked pseudo-seed, and the capacity of the job's two streams
    uint32_t g_a, g_b, t0, t1, row_cap, lnk_cap;
    uint64_t hdr_off, lnk_off;
};

// K12a's jobs of one round: runs of regions of about job_cols columns (each region with the 'N' column in front of it); a job
// starts only behind a region that has columns (its rows' first tags come from the tail of that region's alignments).
// Capacities: cell rows = columns + the longest insertion run after every column -- bounded by the candidates' bases, in
// practice a fraction of the columns: three times the columns are laid out, a job that needs more declines the pile (host
// path); links <= tags = the alignments' columns (<= q_len + t_len each) + a tag per row of an unaligned region's columns
// + `rows` per 'N'.  The jobs are appended to out; hdr_words / lnk_words run on from one round of a call to the next.
inline void cut_lq_jobs(const std::vector<LqRegionLoad> &regs, uint64_t job_cols, uint32_t rows, uint64_t &hdr_words, uint64_t &lnk_words,
                        std::vector<LqJobCut> &out) {
    const uint32_t nr = (uint32_t)regs.size();
    for (uint32_t g = 0, t = 0; g < nr;) {
        LqJobCut jb{g, 0, t, 0, 0, 0, hdr_words, lnk_words};
        uint64_t cols = 0, ins = 0, tags = 0;
        do {
            const LqRegionLoad &R = regs[g];
            cols += (uint64_t)R.sl + 1;
            ins += R.q_bases;
            tags += rows + R.qt_bases + (uint64_t)R.empty_rows * R.sl;
            t += R.sl + 1;
            g++;
        } while (g < nr && (cols < job_cols || regs[g - 1].sl == 0));
        jb.g_b = g;
        if (g == nr) cols += 1, tags += rows, t += 1;  // the closing 'N'
        jb.t1 = t;
        jb.row_cap = (uint32_t)std::min<uint64_t>(cols + ins, 3 * cols + 256);
        jb.lnk_cap = (uint32_t)std::min<uint64_t>(tags, (uint64_t)jb.row_cap * rows);
        hdr_words += jb.row_cap;
        lnk_words += jb.lnk_cap;
        out.push_back(jb);
    }
}

struct PoaLoad {     // one problem of a POA round
    uint64_t cells;  // (X + 1)(Y + 1) of its alignment
    uint64_t rows;   // X: nodes of its graph
};
constexpr uint64_t kPoaMaxRows = 65535;  // a route names a row in 16 bits

// The next launch of a round, from problem a on: as many as fit the budget of cells.  A problem over the budget on its own, or of
// more than kPoaMaxRows rows, goes to `dropped` (it leaves the device path) and the cut goes on behind it.  Returns where the
// launch after this one starts; slice may come back empty (everything from a on was dropped).
inline size_t next_poa_slice(const std::vector<PoaLoad> &load, size_t a, uint64_t budget, std::vector<size_t> &slice, std::vector<size_t> &dropped) {
    slice.clear(), dropped.clear();
    uint64_t cells = 0;
    for (; a < load.size(); a++) {
        if (load[a].cells > budget || load[a].rows > kPoaMaxRows) {
            dropped.push_back(a);
            continue;
        }
        if (!slice.empty() && cells + load[a].cells > budget) break;
        cells += load[a].cells;
        slice.push_back(a);
    }
    return a;
}

}  // namespace ndgpu
