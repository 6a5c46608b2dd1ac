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

// ---- the arena of a resident POA graph (K19: the poa_graph_* kernels of lq_kernels.hip, run_poa's resident form) ----
// One arena per problem, laid out once from a bound the host computes before the first launch: a sequence of Y bytes adds at most
// Y + 1 nodes (its bases and the NUL of the tail chain) and at most Y + 1 edges, so bound = sum(len_k + 1) holds every node and every
// edge the problem can ever have.  Ids are 16 bits with 0xffff for "none", hence bound <= 65,535 (ids 0 .. 65,534).
// Every part starts at a multiple of 8 bytes, so that the tables K13 reads (rows, predecessor rows, route) have whole element
// offsets from the batch's arena base.  Pure 64-bit arithmetic; the kernels compute the same layout from the same bound.
#if defined(__HIPCC__)
#define NDGPU_PLAN_HD __host__ __device__
#else
#define NDGPU_PLAN_HD
#endif
constexpr uint64_t kPoaArenaMaxBound = 65535;
enum PoaPart : int {
    kPaLabels,    // uint64 [bound]      per edge: bit i = sequence i walks it
    kPaScore,     // double [bound]      per node: the heaviest path's score
    kPaRows,      // 8 bytes [bound]     PoaRowDev, what K13 reads
    kPaRoute,     // uint32 [bound]      K13's route words (X + Y <= bound of them)
    kPaNIn,       // uint16 [bound]      per node: in-degree
    kPaInHead, kPaInTail, kPaOutHead, kPaOutTail,   // uint16 [bound] per node: its in-edge / out-edge list in insertion order
    kPaAlHead, kPaAlNext, kPaAlTail,                // uint16 [bound] per node: its column's oldest node, the next younger one; per oldest node: the youngest
    kPaEFrom, kPaETo, kPaENextIn, kPaENextOut,      // uint16 [bound] per edge
    kPaOrder, kPaRank, kPaGrpOf, kPaGrpHead, kPaPrev,   // uint16 [bound]
    kPaPreds,     // uint16 [2 bound]    predecessor rows: sum over rows of max(in-degree, 1) <= nodes + edges
    kPaStack,     // uint16 [2 bound + 2] the DFS stack: one root, a group per started group, a group per out-edge
    kPaBase, kPaDone, kPaStarted,                   // uint8 [bound]
    kPaCount
};
struct PoaArena {
    uint64_t bound;
    uint64_t off[kPaCount];   // bytes from the problem's arena base
    uint64_t len[kPaCount];   // bytes of the part
    uint64_t bytes;           // of the whole arena (a multiple of 8)
};
// false (nothing written): bound 0 or beyond 65,535 -- such a problem does not take the resident path
NDGPU_PLAN_HD inline bool poa_arena_layout(uint64_t bound, PoaArena &A) {
    if (bound == 0 || bound > kPoaArenaMaxBound) return false;
    A.bound = bound;
    uint64_t at = 0;
#pragma unroll   // (device code: the offsets stay in registers)
    for (int p = 0; p < (int)kPaCount; p++) {
        const uint64_t elem = p <= (int)kPaRows ? 8 : p == (int)kPaRoute ? 4 : p <= (int)kPaStack ? 2 : 1;
        const uint64_t count = p == (int)kPaPreds ? 2 * bound : p == (int)kPaStack ? 2 * bound + 2 : bound;
        A.off[p] = at;
        A.len[p] = elem * count;
        at += (A.len[p] + 7) & ~(uint64_t)7;
    }
    A.bytes = at;
    return true;
}
// the arenas of a batch back to back: off[i] = first byte of problem i's arena; returns the total.  A bound that has no layout
// takes no room (off[i] = the next problem's).
inline uint64_t poa_arena_offsets(const uint64_t *bounds, size_t n, uint64_t *off) {
    uint64_t at = 0;
    for (size_t i = 0; i < n; i++) {
        PoaArena A;
        off[i] = at;
        if (poa_arena_layout(bounds[i], A)) at += A.bytes;
    }
    return at;
}

}  // namespace ndgpu
