// Low-quality-region rounds on the device (gfx950, wave64).
//
// The reference re-assembles every low-quality region of a seed from the pile: <= 30 candidate sequences per region are
// aligned to the region's pseudo-seed, the regions are joined with 'N' columns into one linked pseudo-seed, and a second,
// small MSA over these <= 30 rows is scored and walked (generate_consensus_trimed, lib/nextcorrect.c:1538-1669;
// get_lqseqs_from_align_tags, :1250-1338: six symbols, plain maximum, factor 2 / HiFi 4, origin = the last cell); twice
// per seed (iterate_generate_consensus_trimed, :1671-1715).  The alignments are on the device already (K7 / K8a); K12 keeps the
// rest here.  Until round 4 K12 was ONE wavefront per pile doing everything column by column (~300 instructions per cell row on a
// chain as long as the pile's regions together): the longest pile of a launch set the launch's length, and under eight contexts'
// load every instruction of that chain waited its turn.  What a cell row's links ARE does not depend on any score -- only which of
// them wins does -- and a region's links depend on the region before it through two tags per row, which the tail of that row's
// alignment gives away.  So:
//
// K12a lq_links  one wavefront per JOB = a run of regions of one pile (each with the 'N' column in front of it; the last job also
//             takes the closing 'N').  Lanes = rows (<= 30, row order = the reference's first-seen order of links).  A lane derives
//             its row's next tag on the fly from the 2-bit column kinds K8a left in HBM and the 2-bit candidate bases (no tag
//             arrays, no strings); per cell row (column, delta) the six cells' (pp, ppp) links are collected in first-seen order
//             with K9's ballot leader loop and written out: a header (links per cell, coverage) and one word per link -- count,
//             the cell of pp, the cell of ppp -- relative to the link's own column, so that the stream means the same wherever
//             the job sits.  Thousands of jobs per launch: throughput work.
// K12b lq_score  one wavefront per pile walks the jobs' streams in order: a link's score = the best score among the links of pp's
//             cell that continue ppp, + 10 x count - factor x coverage (two column tables in LDS), every cell's best link chosen
//             with the reference's sequential tie-break, one word per cell written (cell row and symbol of its best predecessor,
//             whether its own character is confident); then the wavefront walks the best predecessors from the last cell
//             through an LDS window and emits the consensus characters.  ~100 instructions per cell row, its inputs a sequential
//             stream fetched a row ahead.
// A pile that does not fit the LDS tables (an insertion run of >= 48 columns, > 384 links in a column) or whose alignments do
// not end at both sequence ends is declined (err != 0): the host path (consensus.cpp) takes it.
//
// K13 poa_align  the pseudo-seeds themselves: one sequence of a region's POA against its graph, a batch of regions per launch (at the
//             end of this file; DeviceAligner::run_poa drives it in lockstep rounds).
// K14 lq_rank    the 8-mer ranking of a region's candidates, one wavefront per region, behind K11 (after K19 in this file).
// K19 poa_graph_* the POA graph itself, resident from a problem's first sequence to its consensus string: four kernels around K13
//             (behind K13 in this file; DeviceAligner::run_poa's resident form drives them).
#include <hip/hip_runtime.h>

#include <climits>

#include "nd_device.h"
#include "nd_lqplan.h"

namespace ndgpu {

namespace {

constexpr int kLqRows = 30;          // LQSEQ_MAX_CAN_COUNT rows of the second MSA (lib/nextcorrect.h)
constexpr int kLqDeltaCap = 48;      // cell rows per column the LDS tables hold
constexpr int kLqCellCap = 32;       // links per cell (<= 30 rows)
constexpr int kLqWalkRows = 256;     // cell rows the walk stages in LDS at a time
// A cell's record, all the walk needs: the cell row and symbol of its best predecessor and whether its own character is
// confident -- [31:4] cell row (kLqNoRow: none, the walk ends), [3] best_link * qv_factor > coverage, [2:0] symbol.
constexpr uint32_t kLqNoRow = 0xfffffffu;

// A link of the stream K12a writes and K12b reads, one word: [5:0] count; [14:6] cell of pp (delta * 6 + symbol), [15] pp lies in
// the column before the link's own, [16] pp is the head (no predecessor); [25:17] cell of ppp, [27:26] how many columns before the
// link's own ppp lies (0..2), [28] ppp is the head.
constexpr uint32_t kLnkPpHead = 1u << 16, kLnkPppHead = 1u << 28;
// A cell row's header: [35:0] links per cell, six bits each; [41:36] coverage of the column; [42] first cell row of a column.
constexpr uint64_t kHdrD0 = 1ull << 42;

__device__ __forceinline__ uint32_t lq_op_at(const uint32_t *__restrict__ W, uint32_t col) {
    return (W[col >> 4] >> ((col & 15u) * 2u)) & 3u;
}
__device__ __forceinline__ uint32_t lq_code_at(const uint32_t *__restrict__ pool, uint64_t off) {
    return (pool[off >> 4] >> ((uint32_t)(off & 15u) * 2u)) & 3u;
}
// read code (A0 C1 G2 T3) -> consensus code (A0 T1 G2 C3, lib/nextcorrect.c:52-62)
__device__ __forceinline__ uint32_t lq_cns_code(uint32_t c) { return (0x1230u >> (c * 4u)) & 7u; }

// ---------------------------------------------------------------------------------------------------------------------------
// K12a: the links of a job's cell rows
__global__ __launch_bounds__(64) void lq_links_kernel(LqJobDev *__restrict__ jobs, const LqPileDev *__restrict__ piles,
                                                       const LqPieceDev *__restrict__ pieces, const AlnTask *__restrict__ tasks,
                                                       const AlnOut *__restrict__ outs, const uint32_t *__restrict__ ops,
                                                       const uint32_t *__restrict__ pool, uint64_t *__restrict__ hdr_out,
                                                       uint32_t *__restrict__ lnk_out) {
    __shared__ uint32_t l_pp[6][kLqCellCap], l_ppp[6][kLqCellCap], l_cnt[6][kLqCellCap];

    LqJobDev &JD = jobs[blockIdx.x];
    const LqJobDev J = JD;
    const LqPileDev P = piles[J.pile];
    const int lane = (int)threadIdx.x;
    if (P.link_len == 0) {  // a round the host did not lay out (it takes it itself)
        if (lane == 0) JD.err = 9u, JD.n_rows = 0u, JD.n_links = 0u;
        return;
    }
    const bool row_ok = lane < kLqRows;
    const LqPieceDev *__restrict__ my = pieces + P.first_piece + (uint32_t)(row_ok ? lane : 0) * P.n_regions;
    uint64_t *__restrict__ H = hdr_out + J.hdr_off;
    uint32_t *__restrict__ L = lnk_out + J.lnk_off;

    uint32_t err = 0;
    // the lane's row: current piece
    bool aligned = false;
    const uint32_t *W = nullptr;
    uint32_t col = 0, col_end = 0;
    uint64_t qo = 0;
    uint32_t p1 = kTagHead, p2 = kTagHead;  // the row's two previous tags
    // the word of 16 column kinds / 16 bases the row is reading, and the word after it
    uint32_t ops_wi = 0x7fffffffu, ops_w = 0, ops_nx = 0;
    uint64_t q_wi = ~0ull >> 1;
    uint32_t q_w = 0, q_nx = 0;
    auto op_peek = [&]() -> uint32_t {
        const uint32_t wi = col >> 4;
        if (wi != ops_wi) {
            ops_w = wi == ops_wi + 1u ? ops_nx : W[wi];
            ops_wi = wi;
            ops_nx = W[wi + 1u];
        }
        return (ops_w >> ((col & 15u) * 2u)) & 3u;
    };
    auto q_take = [&]() -> uint32_t {
        const uint64_t wi = qo >> 4;
        if (wi != q_wi) {
            q_w = wi == q_wi + 1ull ? q_nx : pool[wi];
            q_wi = wi;
            q_nx = pool[wi + 1ull];
        }
        const uint32_t c = (q_w >> ((uint32_t)(qo & 15u) * 2u)) & 3u;
        qo++;
        return lq_cns_code(c);
    };
    auto load_piece = [&](uint32_t g) {
        aligned = false;
        if (!row_ok) return;
        const LqPieceDev pc = my[g];
        if (pc.task < 0) return;
        const AlnOut O = outs[pc.task];
        if (O.status != ST_ALIGNED || O.n_cols <= 2) return;  // no alignment / the > 250-gap marker: an 'M' row (nextcorrect.c:1601)
        const AlnTask T = tasks[pc.task];
        if (O.x_final != T.q_len || O.y_final != T.t_len) {  // (the reference pads the unaligned tails; a finished sweep has none)
            err = 2;
            return;
        }
        aligned = true;
        W = ops + T.ops_off;
        col = T.ops_cap - (uint32_t)O.n_cols;
        col_end = T.ops_cap;
        qo = T.q_off & kOffMask;
        ops_wi = col >> 4;
        ops_w = W[ops_wi];
        ops_nx = W[ops_wi + 1u];
        q_wi = qo >> 4;
        q_w = pool[q_wi];
        q_nx = pool[q_wi + 1ull];
    };

    // ---- where the rows stand when the job begins: the last two tags of every row in the region before the job's first 'N'
    //      (lib/nextcorrect.c:1601-1640: a row has a tag in every column).  An aligned row's come from the tail of its column
    //      kinds: kind 0 = both bases, 1 = a candidate base hanging on the last column (delta = its place in the run), 2 = a gap.
    if (J.g_a > 0 && row_ok) {
        const uint32_t gp = J.g_a - 1u;
        const uint32_t t_end = J.t0 - 1u;       // last column of region gp (the host starts no job behind an empty region)
        const LqPieceDev pc = my[gp];
        bool al = false;
        AlnOut O;
        AlnTask T;
        if (pc.task >= 0) {
            O = outs[pc.task];
            if (O.status == ST_ALIGNED && O.n_cols > 2) {
                T = tasks[pc.task];
                if (O.x_final != T.q_len || O.y_final != T.t_len) err = 2;
                else al = true;
            }
        }
        if (al) {
            // the job before checks "no columns of the finished piece left over" only where an 'N' column follows INSIDE it; for the
            // region in front of this job that column is this job's first, so the count is taken here: the alignment must hold
            // exactly one kind that is not a hanging base (kind 1) per column of the region
            uint32_t cols_t = 0;
            const uint32_t *Wc = ops + T.ops_off;
            for (uint32_t c = T.ops_cap - (uint32_t)O.n_cols; c < T.ops_cap; c++) cols_t += lq_op_at(Wc, c) != 1u;
            if (cols_t != pc.sl) err = 7;
        }
        if (!al) {
            p1 = tag_pack((int32_t)t_end, 0u, 6u);
            p2 = pc.sl >= 2u ? tag_pack((int32_t)t_end - 1, 0u, 6u) : tag_pack((int32_t)t_end - 1, 0u, 5u);  // (the 'N' in front of a one-column region)
        } else {
            const uint32_t *Wp = ops + T.ops_off;
            const uint32_t c1 = T.ops_cap, c0 = T.ops_cap - (uint32_t)O.n_cols;  // kinds [c0, c1)
            const uint64_t q0 = T.q_off & kOffMask;
            uint32_t qn = (uint32_t)T.q_len;     // candidate bases not yet stepped over, from the end
            // the run of hanging bases the alignment ends with
            uint32_t r = 0;
            while (c1 - r > c0 && lq_op_at(Wp, c1 - 1u - r) == 1u && r <= (uint32_t)kLqDeltaCap) r++;
            if (r > (uint32_t)kLqDeltaCap) err = 4;
            else if (r >= 2u) {
                p1 = tag_pack((int32_t)t_end, r, lq_cns_code(lq_code_at(pool, q0 + qn - 1u)));
                p2 = tag_pack((int32_t)t_end, r - 1u, lq_cns_code(lq_code_at(pool, q0 + qn - 2u)));
            } else {
                uint32_t i = c1 - 1u;            // kind index of the last tag
                if (r == 1u) {
                    p1 = tag_pack((int32_t)t_end, 1u, lq_cns_code(lq_code_at(pool, q0 + qn - 1u)));
                    qn--, i--;
                    const uint32_t k = lq_op_at(Wp, i);  // the column's own tag (kind 0 or 2: the column exists)
                    p2 = tag_pack((int32_t)t_end, 0u, k == 2u ? 4u : lq_cns_code(lq_code_at(pool, q0 + qn - 1u)));
                } else {
                    const uint32_t k = lq_op_at(Wp, i);
                    p1 = tag_pack((int32_t)t_end, 0u, k == 2u ? 4u : lq_cns_code(lq_code_at(pool, q0 + qn - 1u)));
                    if (k == 0u) qn--;
                    i--;                         // (n_cols > 2: there is a kind before)
                    const uint32_t k2 = lq_op_at(Wp, i);
                    if (k2 != 1u) p2 = tag_pack((int32_t)t_end - 1, 0u, k2 == 2u ? 4u : lq_cns_code(lq_code_at(pool, q0 + qn - 1u)));
                    else {                       // a hanging base of the column before (the 'N' column if the region has one column)
                        uint32_t r2 = 0;
                        while (i + 1u - r2 > c0 && lq_op_at(Wp, i - r2) == 1u && r2 <= (uint32_t)kLqDeltaCap) r2++;
                        if (r2 > (uint32_t)kLqDeltaCap) err = 4;
                        p2 = tag_pack((int32_t)t_end - 1, r2, lq_cns_code(lq_code_at(pool, q0 + qn - 1u)));
                    }
                }
            }
        }
    }

    uint32_t row = 0, n_lnk = 0;  // cell rows / links written so far
    uint32_t t = J.t0;            // column
    uint32_t g = J.g_a, c_in = 0; // region coming up and column inside the current one
    bool sep = true;
    uint32_t sl_cur = 0;
    const uint32_t t_stop = J.t1;

    while (t < t_stop && !__ballot(err != 0)) {
        // -------- one column
        uint32_t coverage = 0;
        uint32_t d = 0;
        for (;; d++) {
            // ---- the lane's tag in cell row (t, d), if any
            bool has = false;
            uint32_t base = 0;
            if (d == 0) {
                has = row_ok;
                if (sep) base = 5;
                else if (aligned) {
                    const uint32_t op = col < col_end ? op_peek() : 1u;
                    if (op == 1u) err = 3;   // the row has no column for this target base
                    else {
                        base = op == 0u ? q_take() : 4u;
                        col++;
                    }
                } else base = 6;
            } else if (aligned && col < col_end && op_peek() == 1u) {
                has = true;
                base = q_take();
                col++;
            }
            if (d > 0 && !__ballot(has)) break;
            if (d >= (uint32_t)kLqDeltaCap || row >= J.row_cap) {
                err = 4;
                break;
            }
            const uint32_t cur = tag_pack((int32_t)t, d, base);
            uint32_t pp = kTagHead, ppp = kTagHead;
            if (has) {
                pp = p1;
                ppp = p2;
                p2 = p1;
                p1 = cur;
            }
            if (d == 0) coverage = (uint32_t)__popcll(__ballot(has && base != 6u));  // nextcorrect.c:1525
            const bool counted = has && base != 6u && (pp & 7u) != 6u;   // update_msa skips 'M' tags (nextcorrect.c:222)

            // ---- links of the six cells, first-seen order (K9's leader loop, all six cells in one pass: a link is (base, pp,
            //      ppp), the earliest row that carries an unseen one leads, its cell's list grows by one)
            unsigned long long cnt6 = 0;  // links per cell so far, 8 bits each (the same in every lane)
            {
                unsigned long long rem = __ballot(counted);
                while (rem) {
                    const int ld = __ffsll((long long)rem) - 1;
                    const uint32_t kb = (uint32_t)__builtin_amdgcn_readlane((int)base, ld);
                    const uint32_t kp = (uint32_t)__builtin_amdgcn_readlane((int)pp, ld);
                    const uint32_t kpp = (uint32_t)__builtin_amdgcn_readlane((int)ppp, ld);
                    const bool in_rem = (rem >> lane) & 1ull;
                    const unsigned long long same = __ballot(in_rem && base == kb && pp == kp && ppp == kpp);
                    const uint32_t n0 = (uint32_t)(cnt6 >> (8u * kb)) & 0xffu;
                    if (lane == ld) {
                        l_pp[kb][n0] = kp;
                        l_ppp[kb][n0] = kpp;
                        l_cnt[kb][n0] = (uint32_t)__popcll(same);
                    }
                    cnt6 += 1ull << (8u * kb);
                    rem &= ~same;
                }
            }
            __builtin_amdgcn_wave_barrier();
            uint32_t n_cell[6], st_cell[6];
            uint32_t n_row = 0;
#pragma unroll
            for (uint32_t bb = 0; bb < 6; bb++) {
                n_cell[bb] = (uint32_t)(cnt6 >> (8u * bb)) & 0xffu;
                st_cell[bb] = n_row;
                n_row += n_cell[bb];
            }
            if (n_lnk + n_row > J.lnk_cap) {
                err = 5;
                break;
            }
            // ---- the row's stream: header by lane 0, lane j the row's j-th link (cells in order)
            if (lane == 0)
                H[row] = (uint64_t)n_cell[0] | (uint64_t)n_cell[1] << 6 | (uint64_t)n_cell[2] << 12 | (uint64_t)n_cell[3] << 18 |
                         (uint64_t)n_cell[4] << 24 | (uint64_t)n_cell[5] << 30 | (uint64_t)coverage << 36 | (d == 0 ? kHdrD0 : 0ull);
            if ((uint32_t)lane < n_row) {
                const uint32_t j = (uint32_t)lane;
                const uint32_t bb = (j >= st_cell[1]) + (j >= st_cell[2]) + (j >= st_cell[3]) + (j >= st_cell[4]) + (j >= st_cell[5]);
                // (an empty cell shares its start with the next one: the comparisons step over it)
                const uint32_t k = j - (bb == 0 ? st_cell[0] : bb == 1 ? st_cell[1] : bb == 2 ? st_cell[2] : bb == 3 ? st_cell[3]
                                                 : bb == 4 ? st_cell[4] : st_cell[5]);
                const uint32_t mpp = l_pp[bb][k], mppp = l_ppp[bb][k];
                uint32_t w = l_cnt[bb][k] & 63u;
                if (mpp == kTagHead) w |= kLnkPpHead | kLnkPppHead;
                else {
                    const uint32_t pt = (uint32_t)tag_tpos(mpp);
                    if (pt != t && pt + 1u != t) err = 6;  // (every row has a tag in every column: cannot happen)
                    const uint32_t ci = tag_delta(mpp) * 6u + tag_base(mpp);
                    if (ci >= (uint32_t)kLqDeltaCap * 6u) err = 4;
                    w |= ci << 6 | (pt == t ? 0u : 1u << 15);
                    if (mppp == kTagHead) w |= kLnkPppHead;
                    else {
                        const uint32_t qt = (uint32_t)tag_tpos(mppp);
                        const uint32_t back = t - qt;
                        const uint32_t cj = tag_delta(mppp) * 6u + tag_base(mppp);
                        if (back > 2u) err = 6;
                        if (cj >= (uint32_t)kLqDeltaCap * 6u) err = 4;
                        w |= cj << 17 | (back & 3u) << 26;
                    }
                }
                L[n_lnk + j] = w;
            }
            __builtin_amdgcn_wave_barrier();
            n_lnk += n_row;
            row++;
            // ---- an 'N' column ends a region: the rows move on to their pieces of the next one, whose leading insertions
            //      hang on this column
            if (d == 0 && sep) {
                if (aligned && col != col_end) err = 7;  // columns of the finished piece left over
                if (g < P.n_regions) {
                    load_piece(g);
                    sl_cur = pieces[P.first_piece + g].sl;
                } else aligned = false;
            }
        }
        // ---- next column
        t++;
        if (sep) {
            sep = false;
            c_in = 0;
            if (sl_cur == 0) {  // an empty pseudo-seed: its closing 'N' follows at once
                sep = true;
                g++;
            }
        } else if (++c_in == sl_cur) {
            sep = true;
            g++;
        }
    }
    const unsigned long long eb = __ballot(err != 0);
    const uint32_t e_first = (uint32_t)__shfl((int)err, eb ? __ffsll((long long)eb) - 1 : 0, 64);
    if (lane == 0) {
        JD.n_rows = row;
        JD.n_links = n_lnk;
        JD.err = e_first;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// K12b: scores and best links -- one wavefront per JOB (the same jobs K12a cut: runs of regions of ~192 columns)
//
// A link's score needs the scores of the column before, so a pile's columns are one chain -- until round 4 one wavefront walked it from
// the pile's first column to its last (10 ms per launch at ~1 % of the device, and the last kernel of every step).  The chain is cut
// the way K10 cuts the main scoring DP (msa_kernels.hip): job j > 0 does not know the scores its first column reads, so it starts
// `warm` columns early -- on the tail of job j - 1's stream, which K12a wrote position-independent -- with every unknown predecessor
// score = one constant C.  Within a few dozen columns the best paths of all links of a column have a common ancestor, and from there on
// the scores it holds differ from the true ones by ONE constant; every decision of this DP compares scores with scores.  Nothing of that
// is assumed: the job stores the scores it held for the last column before its own (`spec`) and the ones it computed for its last
// column (`fin`), and lq_stitch_kernel checks job by job that `spec` is the predecessor's `fin` up to one constant (and equal outright
// for the scores that carry no constant: a head link scores its gain, a link nobody continues scores 0, lib/nextcorrect.c:1273-1289),
// and that no comparison of an offset-carrying score with an absolute one (the floor at 0, an absolute link, the -10 a cell's best
// starts from) could have gone the other way: the smallest true offset-carrying candidate of the job exceeds its largest absolute one.
// A job that fails is scored again in the stitch kernel from its predecessor's true scores (NDGPU_K12_FORCE=repair forces that for
// every second job; NDGPU_K12_WARM sets the warm-up).
constexpr uint32_t kLnkAbs = 1u << 31;   // (table copy of a link word) its score carries no constant
constexpr int32_t kLqSpecC = 1 << 29;    // the constant a speculative start gives every unknown predecessor score
constexpr int32_t kLqNone = INT_MIN;

struct LqLds {                            // the scoring tables of one wavefront
    uint32_t lk[2][kLqLinkCap];           // the links of the current column and the one before ...
    int32_t sc[2][kLqLinkCap];            // ... and their scores
    uint16_t cst[2][kLqDeltaCap * 6], cn[2][kLqDeltaCap * 6];
};
struct LqScoreSt {                        // wave-uniform state of a scoring pass (+ two per-lane trackers)
    uint32_t row = 0;                     // global cell row of the next stream row
    uint32_t row_col0 = 0, row_prev0 = 0; // first cell row of this column / of the one before
    int cur_tab = 1;
    uint32_t used_cur = 0, used_prev = 0; // cell rows of the current / the other table's last use
    uint32_t n_tab = 0, d = 0;
    bool any = false;                     // a column has been seen
    bool spec_pending = false, spec_col = false;  // the pass starts without a column before it / this is that first column
    uint32_t err = 0;
    int32_t mn = INT_MAX, mx = 0;         // per lane: smallest offset-carrying candidate, largest absolute value (the floor included)
};

__device__ __forceinline__ void lq_tables_clear(LqLds &T, int lane) {
    for (int i = lane; i < kLqDeltaCap * 6; i += 64) T.cn[0][i] = T.cn[1][i] = 0;
    __builtin_amdgcn_wave_barrier();
}

// Rows [r0, r1) of a job's stream (headers H, links L, `lb` = the first link of row r0).  WRITE: the cell records go out (a job's own
// rows); otherwise the rows only build the tables (warm-up).
template <bool WRITE>
__device__ __forceinline__ void lq_score_rows(LqLds &T, LqScoreSt &S, const uint64_t *__restrict__ H, const uint32_t *__restrict__ L,
                                              uint32_t r0, uint32_t r1, uint32_t lb, uint32_t *__restrict__ rec, int32_t factor,
                                              int32_t qv_factor, int lane) {
    if (r0 >= r1) return;
    uint64_t h_next = H[r0];                      // the row's header and links are fetched a row ahead
    uint32_t w_next = L[lb + (uint32_t)lane];     // (the stream carries 64 words of padding)
    for (uint32_t r = r0; r < r1; r++) {
        const uint64_t h = h_next;
        const uint32_t w = w_next;
        uint32_t n_cell[6], st_cell[6];
        uint32_t n_row = 0;
#pragma unroll
        for (uint32_t bb = 0; bb < 6; bb++) {
            n_cell[bb] = (uint32_t)(h >> (6u * bb)) & 63u;
            st_cell[bb] = n_row;
            n_row += n_cell[bb];
        }
        if (r + 1u < r1) {
            h_next = H[r + 1u];
            w_next = L[lb + n_row + (uint32_t)lane];
        }
        const uint32_t coverage = (uint32_t)(h >> 36) & 63u;
        if (h & kHdrD0) {  // a new column: the tables swap roles
            const uint32_t u = S.d + 1u < (uint32_t)kLqDeltaCap ? S.d + 1u : (uint32_t)kLqDeltaCap;
            if (S.any) {
                S.used_cur = S.used_prev;
                S.used_prev = u;
            }
            S.any = true;
            S.cur_tab ^= 1;
            S.row_prev0 = S.row_col0;
            S.row_col0 = S.row;
            for (uint32_t i = (uint32_t)lane; i < S.used_cur * 6u; i += 64) T.cn[S.cur_tab][i] = 0;
            __builtin_amdgcn_wave_barrier();
            S.n_tab = 0;
            S.d = 0;
            S.spec_col = S.spec_pending;
            S.spec_pending = false;
        } else S.d++;
        if (S.d >= (uint32_t)kLqDeltaCap) {
            S.err = 4;
            break;
        }
        if (S.n_tab + n_row > (uint32_t)kLqLinkCap) {
            S.err = 5;
            break;
        }
        const int cur = S.cur_tab;
        const uint32_t d = S.d, n_tab = S.n_tab;
        const int32_t penalty = factor * (int32_t)coverage;
        if (lane < 6) {
            T.cst[cur][d * 6u + (uint32_t)lane] = (uint16_t)(n_tab + (lane == 0 ? st_cell[0] : lane == 1 ? st_cell[1] : lane == 2 ? st_cell[2]
                                                                      : lane == 3 ? st_cell[3] : lane == 4 ? st_cell[4] : st_cell[5]));
            T.cn[cur][d * 6u + (uint32_t)lane] = (uint16_t)(lane == 0 ? n_cell[0] : lane == 1 ? n_cell[1] : lane == 2 ? n_cell[2]
                                                           : lane == 3 ? n_cell[3] : lane == 4 ? n_cell[4] : n_cell[5]);
        }
        // ---- score every link of the row (nextcorrect.c:1273-1289): lane jj takes the row's jj-th link
        if ((uint32_t)lane < n_row) {
            const int32_t gain = 10 * (int32_t)(w & 63u) - penalty;
            int32_t sc;
            bool ab;
            const uint32_t before = (w >> 15) & 1u;
            if (w & kLnkPpHead) sc = gain, ab = true;
            else if (S.spec_col && before) {  // the column before the pass's first: unknown, every score there = C
                sc = kLqSpecC + gain;
                ab = false;
                S.mn = sc < S.mn ? sc : S.mn;
            } else {
                int32_t b_off = kLqNone, b_abs = kLqNone;
                const int tb = before ? cur ^ 1 : cur;
                const uint32_t ci = (w >> 6) & 511u;
                const uint32_t s0 = T.cst[tb][ci], sn = T.cn[tb][ci];
                // a link of pp's cell continues ppp when ITS pp is ppp: the same cell, as many columns back
                const uint32_t want_head = w & kLnkPppHead;
                const uint32_t want = (w >> 17) & 511u, want_before = ((w >> 26) & 3u) - before;
                for (uint32_t q = s0; q < s0 + sn; q++) {
                    const uint32_t o = T.lk[tb][q];
                    const bool m = want_head ? (o & kLnkPpHead) != 0u
                                             : !(o & kLnkPpHead) && ((o >> 6) & 511u) == want && ((o >> 15) & 1u) == want_before;
                    if (m) {
                        const int32_t s2 = T.sc[tb][q] + gain;
                        if (o & kLnkAbs) b_abs = s2 > b_abs ? s2 : b_abs;
                        else {
                            b_off = s2 > b_off ? s2 : b_off;
                            S.mn = s2 < S.mn ? s2 : S.mn;
                        }
                    }
                }
                if (b_off != kLqNone) {        // (an offset-carrying candidate wins over the floor and over every absolute one -- checked by the stitch)
                    sc = b_off;
                    ab = false;
                    if (b_abs > S.mx) S.mx = b_abs;
                } else {
                    sc = b_abs > 0 ? b_abs : 0;
                    ab = true;
                }
            }
            if (ab && sc > S.mx) S.mx = sc;
            T.lk[cur][n_tab + (uint32_t)lane] = (w & ~kLnkAbs) | (ab ? kLnkAbs : 0u);
            T.sc[cur][n_tab + (uint32_t)lane] = sc;
        }
        __builtin_amdgcn_wave_barrier();
        // ---- every cell's best link, sequential tie-break (nextcorrect.c:1290-1296): lane bb owns cell bb
        if (WRITE && lane < 6) {
            const uint32_t s0 = T.cst[cur][d * 6u + (uint32_t)lane], n = T.cn[cur][d * 6u + (uint32_t)lane];
            int32_t best = -10;
            uint32_t best_w = kLnkPpHead, best_link = 0;
            for (uint32_t k = 0; k < n; k++) {
                const int32_t sc = T.sc[cur][s0 + k];
                const uint32_t o = T.lk[cur][s0 + k];
                const uint32_t pb = (o & kLnkPpHead) ? 0u : ((o >> 6) & 511u) % 6u;   // symbol of pp (the head's tag is 0)
                if (sc > best || (sc == best && pb != 4u)) {
                    best = sc;
                    best_w = o;
                    best_link = o & 63u;
                }
            }
            const uint32_t bci = (best_w >> 6) & 511u;
            const bool head = (best_w & kLnkPpHead) != 0u;
            const uint32_t prow = head ? kLqNoRow : (((best_w >> 15) & 1u) ? S.row_prev0 : S.row_col0) + bci / 6u;
            const uint32_t conf = (int32_t)best_link * qv_factor > (int32_t)coverage ? 8u : 0u;   // nextcorrect.c:1306
            rec[(uint64_t)S.row * 6u + (uint32_t)lane] = prow << 4 | conf | (head ? 0u : bci % 6u);
        }
        __builtin_amdgcn_wave_barrier();
        S.n_tab += n_row;
        lb += n_row;
        S.row++;
    }
}

// Where the last `warm` columns of a job's stream begin: (row, first link of that row); (0, 0) when the job holds no more columns.
__device__ __forceinline__ void lq_warm_start(const uint64_t *__restrict__ H, uint32_t n_rows, uint32_t n_links, uint32_t warm, int lane,
                                              uint32_t &row_out, uint32_t &lnk_out) {
    uint32_t cols = 0, links_behind = 0;  // columns / links of the rows looked at so far (from the end)
    uint32_t hi = n_rows;                 // rows [hi, n_rows) are looked at
    row_out = 0, lnk_out = 0;
    while (hi > 0) {
        const uint32_t lo = hi > 64u ? hi - 64u : 0u;
        const uint32_t r = hi - 1u - (uint32_t)lane;      // lane 0 = the last row of the window
        const bool in = (uint32_t)lane < hi - lo;
        const uint64_t h = in ? H[r] : 0ull;
        uint32_t nl = 0;
#pragma unroll
        for (uint32_t bb = 0; bb < 6; bb++) nl += (uint32_t)(h >> (6u * bb)) & 63u;
        const unsigned long long d0 = __ballot(in && (h & kHdrD0));
        const uint32_t have = (uint32_t)__popcll(d0);
        if (cols + have >= warm) {   // the column that completes the warm-up starts in this window: its D0 row is the (warm - cols)-th set bit
            unsigned long long m = d0;
            for (uint32_t k = 1; k < warm - cols; k++) m &= m - 1ull;
            const int cut = __ffsll((long long)m) - 1;   // lane of that row
            // links of the rows from the cut on: lanes 0..cut of this window + everything behind
            uint32_t v = (lane <= cut) ? nl : 0u;
            for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
            row_out = hi - 1u - (uint32_t)cut;
            lnk_out = n_links - (links_behind + v);
            return;
        }
        cols += have;
        uint32_t v = nl;
        for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
        links_behind += v;
        hi = lo;
    }
}

// global cell row of a job's first row = the rows of the pile's jobs before it
__device__ __forceinline__ uint32_t lq_rows_before(const LqJobDev *__restrict__ jobs, uint32_t first_job, uint32_t jb, int lane) {
    uint32_t v = 0;
    for (uint32_t k = first_job + (uint32_t)lane; k < jb; k += 64) v += jobs[k].n_rows;
    for (int off = 32; off > 0; off >>= 1) v += (uint32_t)__shfl_xor((int)v, off, 64);
    return v;
}

__device__ __forceinline__ int32_t lq_wave_min(int32_t v) {
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ int32_t lq_wave_max(int32_t v) {
    for (int off = 32; off > 0; off >>= 1) {
        const int32_t o = __shfl_xor(v, off, 64);
        v = o > v ? o : v;
    }
    return v;
}

// a job's boundary planes: [spec scores | spec flags | fin scores | fin flags], kLqLinkCap words each
__device__ __forceinline__ int32_t *lq_plane(int32_t *bnd, uint32_t jb, int which) { return bnd + ((uint64_t)jb * 4u + (uint32_t)which) * kLqLinkCap; }

__device__ __forceinline__ void lq_dump_table(const LqLds &T, int tab, uint32_t n, int32_t *__restrict__ sc, int32_t *__restrict__ fl, int lane) {
    for (uint32_t i = (uint32_t)lane; i < n; i += 64) {
        sc[i] = T.sc[tab][i];
        fl[i] = (T.lk[tab][i] & kLnkAbs) ? 1 : 0;
    }
}

__global__ __launch_bounds__(64) void lq_score_kernel(const LqPileDev *__restrict__ piles, LqJobDev *__restrict__ jobs,
                                                       const uint64_t *__restrict__ hdr_in, const uint32_t *__restrict__ lnk_in,
                                                       uint32_t *__restrict__ cell_rec, int32_t *__restrict__ bnd, uint32_t warm) {
    __shared__ LqLds T;
    const uint32_t jb = blockIdx.x;
    LqJobDev &JD = jobs[jb];
    const LqJobDev J = JD;
    const LqPileDev P = piles[J.pile];
    const int lane = (int)threadIdx.x;
    if (P.link_len == 0 || P.n_jobs == 0) return;  // (K12a marked the jobs of such a pile: err 9)
    const bool first = jb == P.first_job;
    if (J.err || (!first && jobs[jb - 1u].err)) {   // the pile is declined (the stitch reports it)
        if (lane == 0) JD.n_spec = JD.n_fin = 0u, JD.score_err = 0u;
        return;
    }
    uint32_t *__restrict__ rec = cell_rec + P.cell_off;
    const uint32_t row0 = lq_rows_before(jobs, P.first_job, jb, lane);
    LqScoreSt S;
    lq_tables_clear(T, lane);
    uint32_t n_spec = 0;
    if (!first) {
        // ---- warm-up on the tail of the job before
        const LqJobDev Jp = jobs[jb - 1u];
        uint32_t wr = 0, wl = 0;
        lq_warm_start(hdr_in + Jp.hdr_off, Jp.n_rows, Jp.n_links, warm, lane, wr, wl);
        S.row = row0 - (Jp.n_rows - wr);
        S.spec_pending = !(wr == 0u && jb - 1u == P.first_job);  // (a warm-up that reaches the pile's first column is exact)
        lq_score_rows<false>(T, S, hdr_in + Jp.hdr_off, lnk_in + Jp.lnk_off, wr, Jp.n_rows, wl, rec, P.factor, P.qv_factor, lane);
        n_spec = S.n_tab;
        lq_dump_table(T, S.cur_tab, n_spec, lq_plane(bnd, jb, 0), lq_plane(bnd, jb, 1), lane);
        S.mn = INT_MAX, S.mx = 0;   // (what the warm-up compared decides nothing that is kept)
    }
    if (!S.err) lq_score_rows<true>(T, S, hdr_in + J.hdr_off, lnk_in + J.lnk_off, 0u, J.n_rows, 0u, rec, P.factor, P.qv_factor, lane);
    lq_dump_table(T, S.cur_tab, S.n_tab, lq_plane(bnd, jb, 2), lq_plane(bnd, jb, 3), lane);
    const int32_t mn = lq_wave_min(S.mn), mx = lq_wave_max(S.mx);
    if (lane == 0) {
        JD.n_spec = n_spec;
        JD.n_fin = S.n_tab;
        JD.mn = mn;
        JD.mx = mx;
        JD.score_err = S.err;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// K12c: the boundary checks, job by job (one wavefront per pile), and the repair of a job that fails one
__global__ __launch_bounds__(64) void lq_stitch_kernel(LqPileDev *__restrict__ piles, LqJobDev *__restrict__ jobs,
                                                        const uint64_t *__restrict__ hdr_in, const uint32_t *__restrict__ lnk_in,
                                                        uint32_t *__restrict__ cell_rec, int32_t *__restrict__ bnd, uint32_t force_repair) {
    __shared__ LqLds T;
    LqPileDev &PD = piles[blockIdx.x];
    const LqPileDev P = PD;
    const int lane = (int)threadIdx.x;
    if (P.link_len == 0 || P.n_jobs == 0) {
        if (lane == 0) PD.err = 9u, PD.out_len = 0u, PD.n_rows = 0u;
        return;
    }
    uint32_t err = 0;
    for (uint32_t j = 0; j < P.n_jobs; j++) {  // (a job that gave up: the pile goes the host way)
        const uint32_t e = jobs[P.first_job + j].err;
        if (e && !err) err = e;
    }
    uint32_t rows = 0, repairs = 0;
    long long off_prev = 0;   // true score = raw + off for the offset-carrying scores of the job before
    for (uint32_t j = 0; j < P.n_jobs && !err; j++) {
        const uint32_t jb = P.first_job + j;
        const LqJobDev J = jobs[jb];
        if (J.score_err) {
            err = J.score_err;
            break;
        }
        long long off = 0;
        if (j > 0) {
            const LqJobDev Jp = jobs[jb - 1u];
            const int32_t *fs = lq_plane(bnd, jb - 1u, 2), *ff = lq_plane(bnd, jb - 1u, 3), *ss = lq_plane(bnd, jb, 0), *sf = lq_plane(bnd, jb, 1);
            bool ok = Jp.n_fin == J.n_spec;
            bool have = false;
            long long dl = 0;
            if (ok) {
                // true score of every link of the boundary column by the job before / as the job held it
                bool bad = false;
                for (uint32_t i0 = 0; i0 < J.n_spec; i0 += 64) {
                    const uint32_t i = i0 + (uint32_t)lane;
                    const bool in = i < J.n_spec;
                    const long long tp = in ? (long long)fs[i] + (ff[i] ? 0ll : off_prev) : 0ll;
                    const bool s_abs = in && sf[i] != 0;
                    if (s_abs && tp != (long long)ss[i]) bad = true;
                    const unsigned long long rel = __ballot(in && !s_abs);
                    if (rel) {
                        const int ld = __ffsll((long long)rel) - 1;
                        const long long mine = tp - (long long)ss[in ? i : 0];
                        const long long d0 = (long long)(((unsigned long long)(uint32_t)__shfl((int)(mine >> 32), ld, 64) << 32) | (uint32_t)__shfl((int)(uint32_t)mine, ld, 64));
                        if (!have) dl = d0, have = true;
                        if (in && !s_abs && mine != dl) bad = true;
                    }
                }
                ok = !__ballot(bad);
            }
            off = have ? dl : 0ll;
            // no comparison of an offset-carrying candidate with an absolute value went the other way in truth
            if (ok && J.mn != INT_MAX && !((long long)J.mn + off > (long long)J.mx)) ok = false;
            if (force_repair && (j % force_repair) == 1u) ok = false;
            if (!ok) {
                // ---- repair: the boundary column's links once more (their layout), the true scores of the job before put in their
                //      place, then the job's own rows -- exact, every score absolute
                repairs++;
                LqScoreSt S;
                lq_tables_clear(T, lane);
                uint32_t wr = 0, wl = 0;
                lq_warm_start(hdr_in + Jp.hdr_off, Jp.n_rows, Jp.n_links, 1u, lane, wr, wl);
                S.row = rows - (Jp.n_rows - wr);
                S.spec_pending = true;
                lq_score_rows<false>(T, S, hdr_in + Jp.hdr_off, lnk_in + Jp.lnk_off, wr, Jp.n_rows, wl, cell_rec + P.cell_off, P.factor, P.qv_factor, lane);
                if (S.err || S.n_tab != Jp.n_fin) err = S.err ? S.err : 10u;
                else {
                    for (uint32_t i = (uint32_t)lane; i < S.n_tab; i += 64) {
                        T.sc[S.cur_tab][i] = (int32_t)((long long)fs[i] + (ff[i] ? 0ll : off_prev));
                        T.lk[S.cur_tab][i] |= kLnkAbs;
                    }
                    __builtin_amdgcn_wave_barrier();
                    S.mn = INT_MAX, S.mx = 0;
                    lq_score_rows<true>(T, S, hdr_in + J.hdr_off, lnk_in + J.lnk_off, 0u, J.n_rows, 0u, cell_rec + P.cell_off, P.factor, P.qv_factor, lane);
                    if (S.err) err = S.err;
                    lq_dump_table(T, S.cur_tab, S.n_tab, lq_plane(bnd, jb, 2), lq_plane(bnd, jb, 3), lane);
                    __threadfence();
                    if (lane == 0) jobs[jb].n_fin = S.n_tab;
                    __builtin_amdgcn_wave_barrier();
                }
                off = 0;
            }
        }
        if (lane == 0) jobs[jb].row0 = rows;
        off_prev = off;
        rows += J.n_rows;
    }
    if (lane == 0) {
        PD.err = err;
        PD.n_rows = rows;
        PD.n_repair = repairs;
        if (err) PD.out_len = 0u;
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// K12d: the walk (nextcorrect.c:1302-1318), one wavefront per job.  Every row's tags pass through the 'N' cell of every 'N' column (a
// row's tag after (t, d) is (t, d + 1) or (t + 1, 0), and (t, 0) of an 'N' column is the 'N' for every row), so the best-predecessor
// walk from the pile's last cell visits the 'N' cell in front of every job: a job's stretch of it starts at the best predecessor of the
// next job's first cell (the pile's last cell for the last job) and ends with its own first cell.  The characters go to the job's
// stretch of a scratch array in walk order; lq_gather_kernel strings the stretches together, last job first.
__global__ __launch_bounds__(64) void lq_walk_kernel(const LqPileDev *__restrict__ piles, LqJobDev *__restrict__ jobs,
                                                      const uint32_t *__restrict__ cell_rec, char *__restrict__ tmp_chars) {
    __shared__ uint32_t win[kLqWalkRows * 6];    // the walk's window of cell records
    const uint32_t jb = blockIdx.x;
    LqJobDev &JD = jobs[jb];
    const LqJobDev J = JD;
    const LqPileDev P = piles[J.pile];
    const int lane = (int)threadIdx.x;
    if (P.link_len == 0 || P.n_jobs == 0 || P.err) {
        if (lane == 0) JD.out_len = 0u, JD.walk_err = 0u, JD.walk_end = 0u;
        return;
    }
    const uint32_t *__restrict__ rec = cell_rec + P.cell_off;
    char *__restrict__ out = tmp_chars + P.cell_off / 6u + J.row0;
    const uint32_t first = J.row0, end = J.row0 + J.n_rows;
    uint32_t err = 0, out_len = 0;
    uint32_t wrow, wb;
    bool ended = false;   // the walk found a cell without a predecessor here: nothing before it belongs to the consensus
    if (jb + 1u == P.first_job + P.n_jobs) wrow = end - 1u, wb = 5u;   // the origin: the pile's last cell
    else {
        const uint32_t v0 = rec[(uint64_t)end * 6u + 5u];               // the 'N' cell in front of the next job
        wrow = v0 >> 4, wb = v0 & 7u;
        if (wrow == kLqNoRow) ended = true, wrow = first;               // (no row reaches that 'N' with a counted link: the walk ends there)
        else if (wrow >= end || wrow < first) err = 11, wrow = first;
    }
    uint32_t w_lo = end;
    // Every lane walks (the state is uniform), the records come through an LDS window of kLqWalkRows cell rows filled with coalesced
    // loads -- a predecessor is always an earlier row -- and lane 0 writes the characters.
    while (!err && !ended) {
        if (wrow < w_lo) {
            const uint32_t hi = wrow + 1u, lo = hi > first + (uint32_t)kLqWalkRows ? hi - (uint32_t)kLqWalkRows : first;
            __builtin_amdgcn_wave_barrier();
            for (uint32_t i = (uint32_t)lane; i < (hi - lo) * 6u; i += 64) win[i] = rec[(uint64_t)lo * 6u + i];
            __builtin_amdgcn_wave_barrier();
            w_lo = lo;
        }
        const uint32_t v = win[(wrow - w_lo) * 6u + wb];
        if (wb != 4u) {
            if (out_len >= J.n_rows) {
                err = 8;
                break;
            }
            const char ch = wb == 0u ? 'A' : wb == 1u ? 'T' : wb == 2u ? 'G' : wb == 3u ? 'C' : 'N';
            if (lane == 0) out[out_len] = ((v & 8u) || wb == 5u) ? ch : (char)(ch + 32);
            out_len++;
        }
        if ((v >> 4) == kLqNoRow) {                 // no predecessor (the pile's first cell; an 'N' no row reaches with a counted link):
            ended = true;                           // the walk ends (nextcorrect.c:1302-1318)
            break;
        }
        if (wrow == first && wb == 5u) break;      // the job's own first cell: the stretch ends (its predecessor is the job before's)
        wrow = v >> 4;
        wb = v & 7u;
        if (wrow < first) err = 11;                 // left the job without meeting its first cell: cannot happen
    }
    if (lane == 0) JD.out_len = out_len, JD.walk_err = err, JD.walk_end = ended ? 1u : 0u;
}

// K12e: the pile's characters = its jobs' stretches, last job first (walk order)
__global__ __launch_bounds__(64) void lq_gather_kernel(LqPileDev *__restrict__ piles, const LqJobDev *__restrict__ jobs,
                                                        const char *__restrict__ tmp_chars, char *__restrict__ out_chars) {
    LqPileDev &PD = piles[blockIdx.x];
    const LqPileDev P = PD;
    const int lane = (int)threadIdx.x;
    if (P.link_len == 0 || P.n_jobs == 0 || P.err) return;
    uint32_t err = 0;
    uint64_t total = 0;
    uint32_t j_stop = 0;   // the job the walk ends in
    for (uint32_t j = P.n_jobs; j-- > 0;) {
        const LqJobDev &J = jobs[P.first_job + j];
        if (J.walk_err && !err) err = J.walk_err;
        total += J.out_len;
        if (J.walk_end) {
            j_stop = j;
            break;
        }
    }
    if (!err && total > P.out_cap) err = 8;
    if (err) {
        if (lane == 0) PD.err = err, PD.out_len = 0u;
        return;
    }
    char *__restrict__ out = out_chars + P.out_off;
    uint32_t at = 0;
    for (uint32_t j = P.n_jobs; j-- > j_stop;) {
        const LqJobDev &J = jobs[P.first_job + j];
        const char *__restrict__ src = tmp_chars + P.cell_off / 6u + J.row0;
        for (uint32_t i = (uint32_t)lane; i < J.out_len; i += 64) out[at + i] = src[i];
        at += J.out_len;
    }
    if (lane == 0) PD.out_len = at;
}


// ---------------------------------------------------------------------------------------------------------------------------
// K13: POA -- one sequence against the graph (poa.cpp: Graph::align; lib/dag.c:88-134, 261-343), the step of the pseudo-seed
// consensus that costs O(X * Y).  The host hands over the query bytes and, per row in topological order, the node's byte, its
// predecessor rows in in-edge insertion order (row 0 alone when it has none) and whether it has an out-edge; the kernel fills the
// scores S (int32) and the origins F (uint16: [1:0] kind, [15:2] which in-edge) in HBM, picks the best sink row -- the first in
// topological order with the strictly greatest last-column score -- walks back and returns the route, nothing else.
//
// A row: lane l of a 64-column chunk owns column j.  The candidates through the in-edges read finished rows only -- per edge the
// deletion (the cell above-right + gap) beats the match (the cell above + 1 / - 2, bases compared as bytes) on >=, a later edge
// replaces an earlier one only when strictly greater: cv[j], ct[j].  The one dependence along the row is
//     row[j + 1] = max(cv[j], row[j] - 2), the horizontal move keeping ties (poa.cpp: `up = cv[j] > h`),
// and with a[j] = cv[j] + 2(j + 1), R[j] = row[j] + 2j it is R[j + 1] = max(a[j], R[j]): R[j] = max(R[0], a[0 .. j - 1]), the exclusive
// prefix maximum E[j]; the cell takes its candidate exactly when a[j] > E[j] (strictly: the tie is the horizontal move's).  Six
// data-parallel-primitive moves give the prefix maximum of a chunk, one more shifts it by a lane, and the chunk's last value is the
// carry into the next chunk.
//
// Two forms.  NW = 1: one wavefront per job walks the row chunk by chunk (most regions are a few hundred bases; thousands of jobs
// are resident and hide each other's row-to-row latency).  NW = kPoaGroupWaves: one workgroup per job, wave w owns a fixed segment
// [c0, c1) of every row (whole chunks): it stores its raw candidates and publishes its segment's maximum of a[] (wave 0 folds the
// row's column 0 in), ONE barrier, then every wave knows its carry-in = the maximum of the segments before it and finishes its
// cells.  A wave reads other rows only inside cells [c0, c1]: cells (c0, c1] are its own stores, and cell c0 -- the last cell of the
// wave before -- equals its carry-in, so of the row just finished it keeps that cell in a register and never waits for a
// neighbour's store that no barrier has covered yet (older rows' cell c0 lies behind a barrier).
constexpr int32_t kPoaGap = -2;
constexpr int32_t kPoaNeg = INT_MIN / 2;
enum : uint32_t { kPoaH = 0, kPoaMat = 1, kPoaDel = 2, kPoaOrigin = 3 };   // (poa.cpp: FROM_*)

__device__ __forceinline__ int32_t poa_max(int32_t a, int32_t b) { return a > b ? a : b; }
// inclusive prefix maximum over the 64 lanes
__device__ __forceinline__ int32_t poa_prefix_max(int32_t v) {
    v = poa_max(v, __builtin_amdgcn_update_dpp(kPoaNeg, v, 0x111, 0xf, 0xf, false));  // row_shr:1
    v = poa_max(v, __builtin_amdgcn_update_dpp(kPoaNeg, v, 0x112, 0xf, 0xf, false));  // row_shr:2
    v = poa_max(v, __builtin_amdgcn_update_dpp(kPoaNeg, v, 0x114, 0xf, 0xf, false));  // row_shr:4
    v = poa_max(v, __builtin_amdgcn_update_dpp(kPoaNeg, v, 0x118, 0xf, 0xf, false));  // row_shr:8: every row of 16 scanned
    v = poa_max(v, __builtin_amdgcn_update_dpp(kPoaNeg, v, 0x142, 0xa, 0xf, false));  // row_bcast:15 into rows 1 and 3
    v = poa_max(v, __builtin_amdgcn_update_dpp(kPoaNeg, v, 0x143, 0xc, 0xf, false));  // row_bcast:31 into rows 2 and 3
    return v;
}

template <int NW>
__global__ __launch_bounds__(NW * 64) void poa_align_kernel(PoaJobDev *__restrict__ jobs, const uint32_t *__restrict__ ids,
                                                            const char *__restrict__ qpool, const PoaRowDev *__restrict__ rows,
                                                            const uint16_t *__restrict__ preds, int32_t *S_all, uint16_t *F_all,
                                                            uint32_t *__restrict__ route_all) {
    __shared__ int32_t seg_max[2][NW];
    __shared__ int32_t s_bx;
    PoaJobDev &JD = jobs[ids[blockIdx.x]];
    const PoaJobDev J = JD;
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int X = (int)J.X, Y = (int)J.Y;
    const uint64_t W = (uint64_t)Y + 1u;
    int32_t *const S = S_all + J.cell_off;
    uint16_t *const F = F_all + J.cell_off;
    const unsigned char *__restrict__ q = (const unsigned char *)qpool + J.q_off;
    const PoaRowDev *__restrict__ R = rows + J.row_off;
    const uint16_t *__restrict__ P = preds + J.pred_off;
    // the wave's columns [c0, c1) (cells c0 + 1 .. c1); a wave behind the row's end has none
    const int seg = NW == 1 ? ((Y + 63) & ~63) : ((((Y + NW - 1) / NW) + 63) & ~63);
    const int c0 = wave * seg, c1 = c0 + seg < Y ? c0 + seg : Y;
    const bool own_last = c0 < Y && c1 == Y && lane == ((Y - 1 - c0) & 63);   // the thread of the row's last cell

    // row 0 (dag.c:88-134): the boundary cells point at the origin
    for (int c = tid; c <= Y; c += NW * 64) S[c] = c * kPoaGap, F[c] = (uint16_t)kPoaOrigin;
    if (NW == 1) {
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
    } else __syncthreads();

    int32_t best = 0, edge_prev = c0 * kPoaGap;   // edge_prev (NW > 1): cell c0 of the row just finished (row 0 to begin with)
    int bx = 0;
    bool any = false;
    for (int i = 0; i < X; i++) {
        const PoaRowDev rw = R[i];
        int32_t *const row = S + (uint64_t)(i + 1) * W;
        uint16_t *const frow = F + (uint64_t)(i + 1) * W;
        const uint16_t *__restrict__ pr = P + rw.pred_off;
        const uint32_t base = rw.base;
        // column 0: the best of the predecessors' column 0 + gap (wave 0; the others meet it in their carry-in)
        int32_t carry = kPoaNeg;
        if (wave == 0) {
            int32_t b = S[(uint64_t)pr[0] * W];
            for (uint32_t k = 1; k < rw.n_pred; k++) {
                const int32_t t = S[(uint64_t)pr[k] * W];
                b = t > b ? t : b;
            }
            carry = b + kPoaGap;
            if (lane == 0) frow[0] = (uint16_t)kPoaOrigin;
        }
        // ---- the candidates through the in-edges, chunk by chunk
        int32_t m = kPoaNeg;   // NW > 1: the segment's maximum of a[]
        for (int c = c0; c < c1; c += 64) {
            const int j = c + lane;
            const bool in = j < c1;
            int32_t cv = kPoaNeg;
            uint32_t ct = 0;
            if (in) {
                const uint32_t qb = q[j];
                for (uint32_t k = 0; k < rw.n_pred; k++) {
                    const int32_t *prev = S + (uint64_t)pr[k] * W;
                    const int32_t del = prev[j + 1] + kPoaGap;
                    const int32_t left = (NW > 1 && j == c0 && (int)pr[k] == i) ? edge_prev : prev[j];
                    const int32_t mat = left + (qb == base ? 1 : -2);
                    const bool d = del >= mat;
                    const int32_t cand = d ? del : mat;
                    if (k == 0 || cand > cv) cv = cand, ct = k << 2 | (d ? kPoaDel : kPoaMat);
                }
            }
            const int32_t a = in ? cv + 2 * (j + 1) : kPoaNeg;
            if (NW == 1) {
                // ---- and the horizontal move at once: exclusive prefix maximum, the carry in lane 0
                const int32_t incl = poa_prefix_max(a);
                const int32_t e = poa_max(__builtin_amdgcn_update_dpp(carry, incl, 0x138, 0xf, 0xf, false), carry);  // wave_shr:1
                const bool up = a > e;
                const int32_t r = (up ? a : e) - 2 * (j + 1);
                if (in) {
                    row[j + 1] = r;
                    frow[j + 1] = (uint16_t)(up ? ct : kPoaH);
                }
                if (c == 0 && lane == 0) row[0] = carry;
                if (own_last && j == Y - 1 && rw.sink && (!any || r > best)) bx = i + 1, best = r, any = true;
                carry = poa_max(__builtin_amdgcn_readlane(incl, 63), carry);
            } else {
                if (in) {
                    row[j + 1] = cv;
                    frow[j + 1] = (uint16_t)ct;
                }
                m = a > m ? a : m;
            }
        }
        if (NW > 1) {
            // ---- one exchange per row: every wave's segment maximum (wave 0's with column 0 folded in)
            const int32_t mw = poa_max(__builtin_amdgcn_readlane(poa_prefix_max(m), 63), carry);
            if (lane == 0) seg_max[i & 1][wave] = mw;
            __syncthreads();
            for (int w = 0; w < wave; w++) carry = poa_max(carry, seg_max[i & 1][w]);
            edge_prev = carry - 2 * c0;
            if (wave == 0 && lane == 0) row[0] = carry;
            for (int c = c0; c < c1; c += 64) {
                const int j = c + lane;
                const bool in = j < c1;
                const int32_t cv = in ? row[j + 1] : kPoaNeg;     // (this thread's own stores)
                const uint32_t ct = in ? frow[j + 1] : 0u;
                const int32_t a = in ? cv + 2 * (j + 1) : kPoaNeg;
                const int32_t incl = poa_prefix_max(a);
                const int32_t e = poa_max(__builtin_amdgcn_update_dpp(carry, incl, 0x138, 0xf, 0xf, false), carry);  // wave_shr:1
                const bool up = a > e;
                const int32_t r = (up ? a : e) - 2 * (j + 1);
                if (in) {
                    row[j + 1] = r;
                    frow[j + 1] = (uint16_t)(up ? ct : kPoaH);
                }
                if (own_last && j == Y - 1 && rw.sink && (!any || r > best)) bx = i + 1, best = r, any = true;
                carry = poa_max(__builtin_amdgcn_readlane(incl, 63), carry);
            }
        }
        // the next row reads this one: the lanes of a wave read each other's cells (and only those, see above)
        __threadfence_block();
        __builtin_amdgcn_wave_barrier();
    }
    // ---- dag.c:302-313 the best sink row, dag.c:327-343 the route (one thread; the host reverses it)
    if (own_last) s_bx = bx;
    __syncthreads();
    if (tid == 0) {
        uint32_t *__restrict__ rt = route_all + J.route_off;
        uint32_t n = 0;
        const uint32_t cap = J.X + J.Y;
        int x = s_bx, y = Y;
        while ((x | y) != 0 && n < cap) {
            const uint32_t f = F[(uint64_t)x * W + (uint64_t)y];
            int nx = 0, ny = 0;   // (kPoaOrigin)
            const uint32_t kind = f & 3u;
            if (kind == kPoaH) nx = x, ny = y - 1;
            else if (kind == kPoaMat) nx = P[R[x - 1].pred_off + (f >> 2)], ny = y - 1;
            else if (kind == kPoaDel) nx = P[R[x - 1].pred_off + (f >> 2)], ny = y;
            rt[n++] = (nx != x ? (uint32_t)x : 0u) | (ny != y ? (uint32_t)y << 16 : 0u);
            x = nx, y = ny;
        }
        JD.route_len = (x | y) != 0 ? 0xffffffffu : n;   // (cannot happen: every step leaves a row or a column)
    }
}

// ---------------------------------------------------------------------------------------------------------------------------
// K19: the POA graph itself (poa.cpp: Graph; lib/dag.c:223-250, 345-508, 555-595), resident in one arena per problem from its first
// sequence to its consensus string (DESIGN.md section 0a''''''''; the arena: poa_arena_layout of nd_lqplan.h).  One wavefront per
// problem, four kernels around K13, which runs unchanged on the tables poa_graph_rows makes:
//   poa_graph_start      the first sequence as a chain, the identity order
//   poa_graph_rows       rank, rows, predecessor rows in in-edge insertion order, sink flags, the PoaJobDev
//   poa_graph_thread     the route K13 left threaded through the graph (set_route + thread_route), then the new order (toposort)
//   poa_graph_consensus  the heaviest path and the string, cut at the first NUL
// The graph: a node's in-edges and out-edges are singly linked lists in insertion order (head and tail per node, next per edge).
// The nodes sharing a column are one list in creation order: al_head = the column's oldest node, al_next = the next younger one.
// poa.cpp keeps per node a vector of the column's OTHER nodes; what its code does with those vectors depends on their order in two
// places only -- the emission and the pushes of toposort, both through the vector of the group's head, the lowest id of the group
// = the oldest node, whose vector is the younger nodes in creation order = this list behind its head -- and otherwise on the set
// (thread_route looks for a byte, and a column never holds a byte twice: a node is created only when no node of the column has it).
// The steps whose ORDER is the contract -- the threading walk, the DFS, the heaviest path -- run on lane 0; what is a map over nodes
// runs on all lanes.  Every data-dependent loop has a trip bound from the arena's capacities and sets the problem's error word when
// it reaches it; a problem with an error word is left alone by every later kernel (K13 gets a job of no rows) and the host path
// computes it.  Hand-overs between lanes inside a kernel are marked "hand-over"; everything else crosses a kernel boundary.
constexpr uint32_t kPoaNil = 0xffffu;

struct PoaG {   // a problem's arena as typed pointers
    uint64_t *labels;
    double *sc;
    PoaRowDev *rows;
    uint32_t *route;
    uint16_t *n_in, *in_head, *in_tail, *out_head, *out_tail, *al_head, *al_next, *al_tail, *e_from, *e_to, *e_next_in, *e_next_out;
    uint16_t *order, *rank, *grp_of, *grp_head, *prev, *preds, *stack;
    uint8_t *base, *done, *started;
    uint64_t rows_off, preds_off, route_off;   // bytes from the batch's arena base
};
__device__ __forceinline__ PoaG poa_g(unsigned char *arena, uint64_t arena_off, uint32_t bound) {
    PoaArena A;
    (void)poa_arena_layout(bound, A);   // (the host admitted the bound)
    unsigned char *p = arena + arena_off;
    PoaG g;
    g.labels = (uint64_t *)(p + A.off[kPaLabels]), g.sc = (double *)(p + A.off[kPaScore]), g.rows = (PoaRowDev *)(p + A.off[kPaRows]);
    g.route = (uint32_t *)(p + A.off[kPaRoute]);
    g.n_in = (uint16_t *)(p + A.off[kPaNIn]), g.in_head = (uint16_t *)(p + A.off[kPaInHead]), g.in_tail = (uint16_t *)(p + A.off[kPaInTail]);
    g.out_head = (uint16_t *)(p + A.off[kPaOutHead]), g.out_tail = (uint16_t *)(p + A.off[kPaOutTail]);
    g.al_head = (uint16_t *)(p + A.off[kPaAlHead]), g.al_next = (uint16_t *)(p + A.off[kPaAlNext]), g.al_tail = (uint16_t *)(p + A.off[kPaAlTail]);
    g.e_from = (uint16_t *)(p + A.off[kPaEFrom]), g.e_to = (uint16_t *)(p + A.off[kPaETo]);
    g.e_next_in = (uint16_t *)(p + A.off[kPaENextIn]), g.e_next_out = (uint16_t *)(p + A.off[kPaENextOut]);
    g.order = (uint16_t *)(p + A.off[kPaOrder]), g.rank = (uint16_t *)(p + A.off[kPaRank]), g.grp_of = (uint16_t *)(p + A.off[kPaGrpOf]);
    g.grp_head = (uint16_t *)(p + A.off[kPaGrpHead]), g.prev = (uint16_t *)(p + A.off[kPaPrev]);
    g.preds = (uint16_t *)(p + A.off[kPaPreds]), g.stack = (uint16_t *)(p + A.off[kPaStack]);
    g.base = p + A.off[kPaBase], g.done = p + A.off[kPaDone], g.started = p + A.off[kPaStarted];
    g.rows_off = arena_off + A.off[kPaRows], g.preds_off = arena_off + A.off[kPaPreds], g.route_off = arena_off + A.off[kPaRoute];
    return g;
}

// inclusive prefix sum over the 64 lanes (the moves of poa_prefix_max)
__device__ __forceinline__ uint32_t poa_prefix_sum(uint32_t u) {
    int v = (int)u;
    v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, false);  // row_shr:1
    v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, false);  // row_shr:2
    v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, false);  // row_shr:4
    v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, false);  // row_shr:8
    v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);  // row_bcast:15 into rows 1 and 3
    v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);  // row_bcast:31 into rows 2 and 3
    return (uint32_t)v;
}
__device__ __forceinline__ uint32_t poa_or_lanes(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v |= (uint32_t)__shfl_xor((int)v, m);
    return v;
}

// PoaGraph::start: node i = byte i of the first sequence, edge i = i -> i + 1 with label bit 0, order = identity; every node alone in
// its column.  A lane writes the records of its own nodes and edges and reads none: the hand-over is the kernel boundary.
__global__ __launch_bounds__(64) void poa_graph_start(PoaGraphDev *graphs, PoaXeDev *xe, unsigned char *arena, const char *seqs,
                                                       const PoaSeqDev *__restrict__ seq_tab) {
    PoaGraphDev &GD = graphs[blockIdx.x];
    const uint32_t lane = threadIdx.x, bound = GD.bound;
    const PoaG G = poa_g(arena, GD.arena_off, bound);
    const PoaSeqDev s0 = seq_tab[GD.seq_first];
    const unsigned char *s = (const unsigned char *)seqs + s0.off;
    const uint32_t err = s0.len > bound ? kPoaErrNodes : 0u;   // (the bound counts len + 1 per sequence: cannot happen)
    const uint32_t n = err ? 0u : s0.len;
    for (uint32_t i = lane; i < n; i += 64) {
        const bool first = i == 0, last = i + 1 == n;
        G.base[i] = s[i];
        G.n_in[i] = first ? 0 : 1;
        G.in_head[i] = G.in_tail[i] = (uint16_t)(first ? kPoaNil : i - 1);
        G.out_head[i] = G.out_tail[i] = (uint16_t)(last ? kPoaNil : i);
        G.al_head[i] = G.al_tail[i] = (uint16_t)i, G.al_next[i] = (uint16_t)kPoaNil;
        G.order[i] = (uint16_t)i;
        if (!last) {
            G.e_from[i] = (uint16_t)i, G.e_to[i] = (uint16_t)(i + 1);
            G.e_next_in[i] = G.e_next_out[i] = (uint16_t)kPoaNil;
            G.labels[i] = 1ull;
        }
    }
    if (lane == 0) {
        GD.n_nodes = n, GD.n_edges = n ? n - 1 : 0u, GD.err = err;
        xe[blockIdx.x] = PoaXeDev{n, err};
    }
}

// Graph::build_rows + export_rows for sequence r of the round's problems: row i + 1 = node order[i].  pred_off is the exclusive prefix
// sum of max(in-degree, 1) over the order (wavefront scan, chunk by chunk); a lane walks its node's in-edge list in insertion order
// (at most in-degree steps) and writes rank[from] + 1 per edge, or row 0 alone.
__global__ __launch_bounds__(64) void poa_graph_rows(PoaGraphDev *graphs, const PoaRoundDev *__restrict__ round, uint32_t r,
                                                      unsigned char *arena, const PoaSeqDev *__restrict__ seq_tab, PoaJobDev *jobs) {
    const PoaRoundDev rd = round[blockIdx.x];
    PoaGraphDev &GD = graphs[rd.prob];
    const uint32_t lane = threadIdx.x, bound = GD.bound;
    const PoaG G = poa_g(arena, GD.arena_off, bound);
    const PoaSeqDev sq = seq_tab[GD.seq_first + r];
    const uint32_t X = GD.err ? 0u : GD.n_nodes;
    uint32_t err = 0;
    for (uint32_t i = lane; i < X; i += 64) G.rank[G.order[i]] = (uint16_t)i;
    // hand-over: the walks below read rank entries that other lanes wrote -- fence + wavefront barrier
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    uint32_t carry = 0;
    for (uint32_t c = 0; c < X; c += 64) {
        const uint32_t i = c + lane;
        const bool in = i < X;
        const uint32_t v = in ? G.order[i] : 0u, nin = in ? G.n_in[v] : 0u, cnt = in ? (nin ? nin : 1u) : 0u;
        const uint32_t incl = poa_prefix_sum(cnt), off = carry + incl - cnt;
        if (in) {
            if (off + cnt > 2u * bound) err |= kPoaErrPreds;   // (the sum is at most nodes + edges: cannot happen)
            else {
                PoaRowDev rw;
                rw.pred_off = off, rw.n_pred = (uint16_t)cnt, rw.base = G.base[v], rw.sink = G.out_head[v] == kPoaNil;
                G.rows[i] = rw;
                if (nin == 0) G.preds[off] = 0;
                else {
                    uint32_t e = G.in_head[v], k = 0;
                    for (; k < nin && e != kPoaNil; k++, e = G.e_next_in[e]) G.preds[off + k] = (uint16_t)(G.rank[G.e_from[e]] + 1u);
                    if (k != nin || e != kPoaNil) err |= kPoaErrList;   // the list and its count disagree
                }
            }
        }
        carry += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
    }
    err = poa_or_lanes(err);
    if (lane == 0) {
        if (err) GD.err |= err;
        PoaJobDev J;
        J.X = err ? 0u : X, J.Y = sq.len;
        J.q_off = sq.off, J.row_off = G.rows_off / sizeof(PoaRowDev), J.pred_off = G.preds_off / sizeof(uint16_t);
        J.cell_off = rd.cell_off, J.route_off = G.route_off / sizeof(uint32_t);
        J.route_len = 0, J.pad_ = 0;
        jobs[rd.prob] = J;   // read by K13 and by poa_graph_thread: kernel boundary
    }
}

// Graph::set_route + thread_route + toposort for sequence r of the round's problems.
__global__ __launch_bounds__(64) void poa_graph_thread(PoaGraphDev *graphs, PoaXeDev *xe, const PoaRoundDev *__restrict__ round, uint32_t r,
                                                        unsigned char *arena, const char *seqs, const PoaSeqDev *__restrict__ seq_tab,
                                                        const PoaJobDev *__restrict__ jobs) {
    const PoaRoundDev rd = round[blockIdx.x];
    PoaGraphDev &GD = graphs[rd.prob];
    const uint32_t lane = threadIdx.x, bound = GD.bound;
    if (GD.err) {   // (uniform) an earlier kernel gave the problem up
        if (lane == 0) xe[rd.prob] = PoaXeDev{GD.n_nodes, GD.err};
        return;
    }
    const PoaG G = poa_g(arena, GD.arena_off, bound);
    const PoaJobDev J = jobs[rd.prob];
    const PoaSeqDev sq = seq_tab[GD.seq_first + r];
    const unsigned char *s = (const unsigned char *)seqs + sq.off;   // s[Y] == NUL
    const uint32_t X = J.X, Y = J.Y, n_route = J.route_len;
    uint32_t err = n_route > X + Y || X != GD.n_nodes ? kPoaErrRoute : 0u;   // (K13's walk did not end: cannot happen)

    // ---- the first and the last query offset the route consumes.  The walk back only ever lowers y, so the offsets of the words that
    // consume one fall strictly along the walk: first = the least, last = the greatest (all lanes, then a butterfly)
    uint32_t q_lo = 0xffffffffu, q_hi = 0;   // y = offset + 1; 0: none
    if (!err)
        for (uint32_t a = lane; a < n_route; a += 64) {
            const uint32_t y = G.route[a] >> 16;
            if (y) q_lo = y < q_lo ? y : q_lo, q_hi = y > q_hi ? y : q_hi;
        }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)q_lo, m), hi = (uint32_t)__shfl_xor((int)q_hi, m);
        q_lo = lo < q_lo ? lo : q_lo, q_hi = hi > q_hi ? hi : q_hi;
    }
    if (q_hi == 0 || q_hi > Y) err |= kPoaErrRoute;   // (a route consumes every query base's column at least once, none beyond Y)

    uint32_t nn = GD.n_nodes, ne = GD.n_edges;
    // ---- thread_route (dag.c:345-401), lane 0: nodes and edges are numbered in the order the walk makes them
    if (lane == 0 && !err) {
        const uint64_t bit = 1ull << r;
        auto add_node = [&](uint32_t b) -> uint32_t {
            if (nn >= bound) {
                err |= kPoaErrNodes;
                return kPoaNil;
            }
            const uint32_t id = nn++;
            G.base[id] = (uint8_t)b, G.n_in[id] = 0;
            G.in_head[id] = G.in_tail[id] = G.out_head[id] = G.out_tail[id] = (uint16_t)kPoaNil;
            G.al_head[id] = G.al_tail[id] = (uint16_t)id, G.al_next[id] = (uint16_t)kPoaNil;
            return id;
        };
        auto add_edge = [&](uint32_t from, uint32_t to) {
            if (ne >= bound || from == kPoaNil || to == kPoaNil) {
                err |= kPoaErrEdges;
                return;
            }
            const uint32_t id = ne++;
            G.e_from[id] = (uint16_t)from, G.e_to[id] = (uint16_t)to, G.labels[id] = bit;
            G.e_next_in[id] = G.e_next_out[id] = (uint16_t)kPoaNil;
            if (G.out_head[from] == kPoaNil) G.out_head[from] = (uint16_t)id;
            else G.e_next_out[G.out_tail[from]] = (uint16_t)id;
            G.out_tail[from] = (uint16_t)id;
            if (G.in_head[to] == kPoaNil) G.in_head[to] = (uint16_t)id;
            else G.e_next_in[G.in_tail[to]] = (uint16_t)id;
            G.in_tail[to] = (uint16_t)id;
            G.n_in[to] = (uint16_t)(G.n_in[to] + 1u);
        };
        // dag.c:236-250: `count` bytes from s[at] on (the tail's last one is the NUL); at most Y + 1 trips
        auto add_chain = [&](uint32_t at, uint32_t count, uint32_t &first, uint32_t &head) {
            for (uint32_t i = 0; i < count && !err; i++) {
                const uint32_t id = add_node(s[at + i]);
                if (first == kPoaNil) first = id;
                else add_edge(head, id);
                head = id;
            }
        };
        const uint32_t start_q = q_lo - 1u, end_q = q_hi - 1u;
        uint32_t first = kPoaNil, head = kPoaNil, tail_first = kPoaNil, tail_last = kPoaNil;
        if (start_q > 0) add_chain(0, start_q, first, head);
        if (end_q + 1u < Y) add_chain(end_q + 1u, Y - end_q, tail_first, tail_last);
        bool prev_new = true;
        for (uint32_t a = n_route; a-- > 0 && !err;) {   // the route forwards = K13's words backwards; n_route <= X + Y trips
            const uint32_t w = G.route[a], x = w & 0xffffu, y = w >> 16;
            if (!y) continue;
            if (x > X) {
                err |= kPoaErrRoute;
                break;
            }
            const uint32_t b = s[y - 1u];
            bool is_new = false;
            uint32_t node;
            if (!x) node = add_node(b), is_new = true;
            else {
                const uint32_t rn = G.order[x - 1u];   // (the order of the alignment: the new one is written below, after the walk)
                if (G.base[rn] == b) node = rn;
                else {
                    uint32_t found = kPoaNil, t = 0;
                    for (uint32_t m = G.al_head[rn]; m != kPoaNil; m = G.al_next[m]) {   // the column: at most `bound` nodes
                        if (++t > bound) {
                            err |= kPoaErrList;
                            break;
                        }
                        if (G.base[m] == b) found = m;
                    }
                    if (found != kPoaNil) node = found;
                    else {
                        node = add_node(b), is_new = true;
                        if (node != kPoaNil) {   // dag.c:190-202, 369-372: the new node joins the column of rn, as its youngest
                            const uint32_t h = G.al_head[rn];
                            G.al_head[node] = (uint16_t)h;
                            G.al_next[G.al_tail[h]] = (uint16_t)node;
                            G.al_tail[h] = (uint16_t)node;
                        }
                    }
                }
            }
            if (err) break;
            if (head != kPoaNil) {
                bool add = is_new || prev_new;
                if (!add) {   // dag.c:223-234 label_existing: every head -> node edge gets the bit; a new edge when there is none
                    add = true;
                    uint32_t t = 0;
                    for (uint32_t e = G.out_head[head]; e != kPoaNil; e = G.e_next_out[e]) {   // at most `bound` edges
                        if (++t > bound) {
                            err |= kPoaErrList;
                            break;
                        }
                        if (G.e_to[e] == node) G.labels[e] |= bit, add = false;
                    }
                }
                if (add) add_edge(head, node);
            }
            head = node, prev_new = is_new;
            if (first == kPoaNil) first = head;
        }
        if (!err && tail_first != kPoaNil) add_edge(head, tail_first);
    }
    // hand-over: lane 0 grew the graph, all lanes read it below -- fence + wavefront barrier; the counts travel by readlane
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    nn = (uint32_t)__builtin_amdgcn_readlane((int)nn, 0), ne = (uint32_t)__builtin_amdgcn_readlane((int)ne, 0);
    err = poa_or_lanes(err);

    // ---- toposort (dag.c:469-508 + 403-467).  Groups in ascending order of their heads = of the columns' oldest nodes (all lanes:
    // a wavefront count of the heads before a node); the flags of a group are cleared by its head's lane
    uint32_t ng = 0;
    if (!err) {
        for (uint32_t c = 0; c < nn; c += 64) {
            const uint32_t i = c + lane;
            const uint32_t hd = i < nn && G.al_head[i] == i ? 1u : 0u;
            const uint32_t incl = poa_prefix_sum(hd), gi = ng + incl - hd;
            if (hd) G.grp_head[gi] = (uint16_t)i, G.grp_of[i] = (uint16_t)gi, G.done[gi] = 0, G.started[gi] = 0;
            ng += (uint32_t)__builtin_amdgcn_readlane((int)incl, 63);
        }
    }
    // hand-over: a younger node of a column reads the group its head's lane just wrote -- fence + wavefront barrier
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    if (!err)
        for (uint32_t i = lane; i < nn; i += 64) {
            const uint32_t h = G.al_head[i];
            if (h != i) G.grp_of[i] = G.grp_of[h];
        }
    // hand-over: lane 0's DFS reads every lane's groups and flags -- fence + wavefront barrier
    __threadfence_block();
    __builtin_amdgcn_wave_barrier();
    if (lane == 0 && !err) {
        // The DFS with the stack discipline of poa.cpp.  `started` is not cleared per root: a started group pushes itself below its
        // successors and is therefore popped again -- finished, its flag reset -- before the stack runs empty.
        const uint32_t stack_cap = 2u * bound + 2u, trip_cap = 3u * bound + 3u;   // pops <= pushes <= roots + groups + edges
        int fill = (int)nn - 1;
        uint32_t scan = 0, trips = 0;
        while (fill >= 0 && !err) {
            uint32_t root = kPoaNil;
            for (; scan < ng && root == kPoaNil; scan++) {   // (`scan` only moves on: at most ng trips over all roots)
                if (G.done[scan]) continue;
                bool pred = false;
                uint32_t t = 0;
                for (uint32_t m = G.grp_head[scan]; m != kPoaNil && !pred; m = G.al_next[m]) {
                    if (++t > bound) {
                        err |= kPoaErrList;
                        break;
                    }
                    pred = G.n_in[m] != 0;
                }
                if (!pred) root = scan;
            }
            if (root == kPoaNil || err) {
                err |= kPoaErrOrder;   // (the reference asserts: unreachable for the graphs built here)
                break;
            }
            uint32_t sp = 0;
            G.stack[sp++] = (uint16_t)root;
            while (sp && !err) {
                if (++trips > trip_cap) {
                    err |= kPoaErrTrips;
                    break;
                }
                const uint32_t g = G.stack[--sp];
                if (G.done[g]) continue;
                const uint32_t h = G.grp_head[g];
                if (G.started[g]) {
                    G.done[g] = 1, G.started[g] = 0;
                    uint32_t t = 0;
                    for (uint32_t m = h; m != kPoaNil; m = G.al_next[m]) {   // the head, then the column's nodes from the oldest on
                        if (++t > bound || fill < 0) {
                            err |= kPoaErrOrder;
                            break;
                        }
                        G.order[fill--] = (uint16_t)m;
                    }
                    continue;
                }
                G.started[g] = 1;
                G.stack[sp++] = (uint16_t)g;   // (sp < stack_cap: it was popped a moment ago)
                uint32_t t = 0;
                for (uint32_t m = h; m != kPoaNil && !err; m = G.al_next[m])
                    for (uint32_t e = G.out_head[m]; e != kPoaNil; e = G.e_next_out[e]) {
                        if (++t > bound) {   // the out-edges of a group: at most `bound` edges
                            err |= kPoaErrList;
                            break;
                        }
                        if (sp >= stack_cap) {
                            err |= kPoaErrStack;
                            break;
                        }
                        G.stack[sp++] = G.grp_of[G.e_to[e]];
                    }
            }
        }
    }
    err = poa_or_lanes(err);
    // the order, the graph and the counts are read by the next round's kernels: kernel boundary
    if (lane == 0) {
        GD.n_nodes = nn, GD.n_edges = ne, GD.err = err;
        xe[rd.prob] = PoaXeDev{nn, err};
    }
}

// Graph::heaviest_path (dag.c:555-595) + the cut at the first NUL, lane 0: scores in doubles -- every value is a multiple of 0.5 far
// below 2^53, exact on the device as on the host -- the first edge of a node always taken, a later one only when strictly greater,
// the best node the first of the order with the strictly greatest score.  `best` runs on from node to node, as in poa.cpp.
__global__ __launch_bounds__(64) void poa_graph_consensus(PoaGraphDev *graphs, const uint32_t *__restrict__ ids, unsigned char *arena,
                                                           char *out_all, uint32_t *out_len) {
    const uint32_t prob = ids[blockIdx.x];
    PoaGraphDev &GD = graphs[prob];
    if (threadIdx.x != 0) return;
    if (GD.err) {
        out_len[prob] = 0xffffffffu;
        return;
    }
    const uint32_t bound = GD.bound, n = GD.n_nodes, nseq = GD.n_seq;
    const PoaG G = poa_g(arena, GD.arena_off, bound);
    const uint64_t mask = nseq >= 64u ? ~0ull : ((1ull << nseq) - 1ull);
    uint32_t err = 0, gnode = kPoaNil;
    double best = -1, gbest = -1;
    for (uint32_t i = 0; i < n && !err; i++) {
        const uint32_t v = G.order[i], nin = G.n_in[v];
        uint32_t bp = kPoaNil;
        if (nin) {
            uint32_t e = G.in_head[v], k = 0;
            for (; k < nin && e != kPoaNil; k++, e = G.e_next_in[e]) {   // at most in-degree trips
                const uint32_t from = G.e_from[e];
                const double sc = G.sc[from] + (double)__popcll(G.labels[e] & mask) - 0.5 * (double)nin;
                if (sc > best || bp == kPoaNil) best = sc, bp = from;
            }
            if (k != nin || e != kPoaNil) err |= kPoaErrList;
        } else best = 0;
        G.sc[v] = best, G.prev[v] = (uint16_t)bp;
        if (best > gbest) gbest = best, gnode = v;
    }
    uint32_t len = 0;
    for (uint32_t m = gnode; m != kPoaNil && !err; m = G.prev[m])   // a path: at most n nodes
        if (++len > n) err |= kPoaErrTrips;
    uint32_t cut = len;
    if (!err) {
        char *out = out_all + GD.out_off;   // (capacity bound >= n >= len)
        uint32_t k = 0;
        for (uint32_t m = gnode; m != kPoaNil && k < len; m = G.prev[m], k++) {
            const uint32_t b = G.base[m], at = len - 1u - k;
            out[at] = (char)b;
            if (!b) cut = at;   // (the walk runs backwards: the last one seen is the first NUL of the string)
        }
    }
    if (err) GD.err |= err;
    out_len[prob] = err ? 0xffffffffu : cut;
}

// ---------------------------------------------------------------------------------------------------------------------------
// K14: the 8-mer ranking of a region's candidates (consensus.cpp: lq_rank_host; lib/nextcorrect.c:281-337, 405-440), one wavefront
// per region, right behind K11 on the strings K11 left in the pool (or on the pool of a batch of problems: DeviceAligner::run_rank).
// A sequence gives min(len, 40) - 8 k-mers of its head window (offset 0) or its tail window (offset len - 40 beyond 40 bases), each
// the 16 low bits of eight 3-bit codes shifted by two -- codes of 4 and more spill into the neighbour, as in the reference.
// A pass counts the k-mers of the first min(n, c) sequences of the current order and scores every sequence with the sum of its own
// k-mers' counts.  The reference counts in a 65,536-bin histogram; a pass touches at most 10 x 32 distinct k-mers, so the counts
// live in a 512-slot open-addressing table in LDS (key and count in one word, filled with atomicCAS / atomicAdd: sums, whatever the
// lane order).  The stable sort is a rank by counting: scores greater + equal scores earlier in the current order.
// LDS: 1,600 B codes + 2,560 B k-mers + 2,048 B table + 400 B per-sequence state; the tail windows are staged over the head
// windows, and only in the regions that take the tail pass.
constexpr int kRankMax = 40, kRankWin = 40, kRankK = 8, kRankKm = kRankWin - kRankK, kRankTop = 10, kRankSlots = 512;

struct RankLds {
    uint32_t tab[kRankSlots];              // [31:16] k-mer, [15:0] count; 0: empty
    uint32_t off[kRankMax];                // input order: pool offset, length
    uint16_t len[kRankMax];
    uint16_t km[kRankMax * kRankKm];       // input order: the staged window's k-mers
    uint16_t sc[kRankMax], saved[kRankMax];  // sc: by position; saved: by input index
    uint8_t code[kRankMax * kRankWin];     // input order: the staged window's byte codes
    uint8_t ord[kRankMax];                 // position -> input index
};

// A/a 0, T/t 1, G/g 2, C/c 3, N 5, M 6, any other byte 4 (consensus.cpp: BaseLut)
__device__ __forceinline__ uint32_t rank_code(uint32_t c) {
    const uint32_t u = c & 0xdfu;   // (equals an upper-case letter only for that letter in either case)
    return u == 'A' ? 0u : u == 'T' ? 1u : u == 'G' ? 2u : u == 'C' ? 3u : c == 'N' ? 5u : c == 'M' ? 6u : 4u;
}
__device__ __forceinline__ int rank_nkm(int len) { return len < kRankK ? 0 : (len < kRankWin ? len : kRankWin) - kRankK; }
__device__ __forceinline__ uint32_t rank_slot(uint32_t km) { return (km * 0x9e3bu >> 4) & (uint32_t)(kRankSlots - 1); }

// the window's k-mers of every sequence, input order
__device__ __forceinline__ void rank_stage(RankLds &T, const unsigned char *__restrict__ pool, int n, int from_tail, int lane) {
    for (int i = lane; i < n * kRankWin; i += 64) {
        const int s = i / kRankWin, b = i - s * kRankWin, len = (int)T.len[s];
        const int o = from_tail && len > kRankWin ? len - kRankWin : 0;
        T.code[i] = b < len ? (uint8_t)rank_code(pool[(size_t)T.off[s] + (size_t)(o + b)]) : (uint8_t)0;
    }
    __syncthreads();
    for (int i = lane; i < n * kRankKm; i += 64) {
        const int s = i / kRankKm, k = i - s * kRankKm;
        uint32_t km = 0;
        if (k < rank_nkm((int)T.len[s])) {
            const uint8_t *c = &T.code[s * kRankWin + k];
#pragma unroll
            for (int x = 0; x < kRankK; x++) km = km << 2 | c[x];
        }
        T.km[i] = (uint16_t)km;
    }
    __syncthreads();
}

// count the k-mers of positions [0, min(n, c)), score every position
__device__ __forceinline__ void rank_pass(RankLds &T, int n, int c, int lane) {
    for (int i = lane; i < kRankSlots; i += 64) T.tab[i] = 0u;
    __syncthreads();
    const int lim = n < c ? n : c;
    for (int i = lane; i < lim * kRankKm; i += 64) {
        const int p = i / kRankKm, k = i - p * kRankKm, s = (int)T.ord[p];
        if (k >= rank_nkm((int)T.len[s])) continue;
        const uint32_t km = T.km[s * kRankKm + k];
        for (uint32_t h = rank_slot(km);; h = (h + 1u) & (uint32_t)(kRankSlots - 1)) {   // (<= 320 keys in 512 slots: an empty one exists)
            uint32_t cur = T.tab[h];
            if (cur == 0u) {
                cur = atomicCAS(&T.tab[h], 0u, km << 16 | 1u);
                if (cur == 0u) break;
            }
            if ((cur >> 16) == km) {
                atomicAdd(&T.tab[h], 1u);
                break;
            }
        }
    }
    __syncthreads();
    // a position per half wavefront, a k-mer per lane of it
    for (int i0 = 0; i0 < n * kRankKm; i0 += 64) {
        const int i = i0 + lane, p = i / kRankKm, k = i - p * kRankKm;
        uint32_t v = 0;
        if (p < n) {
            const int s = (int)T.ord[p];
            if (k < rank_nkm((int)T.len[s])) {
                const uint32_t km = T.km[s * kRankKm + k];
                for (uint32_t h = rank_slot(km);; h = (h + 1u) & (uint32_t)(kRankSlots - 1)) {
                    const uint32_t cur = T.tab[h];
                    if (cur == 0u) break;
                    if ((cur >> 16) == km) {
                        v = cur & 0xffffu;
                        break;
                    }
                }
            }
        }
#pragma unroll
        for (int m = kRankKm / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if (p < n && k == 0) T.sc[p] = (uint16_t)v;
    }
    __syncthreads();
}

// stable, descending by score
__device__ __forceinline__ void rank_sort(RankLds &T, int n, int lane) {
    uint32_t s = 0, o = 0, r = 0;
    if (lane < n) {
        s = T.sc[lane], o = T.ord[lane];
        for (int q = 0; q < n; q++) {
            const uint32_t t = T.sc[q];
            r += (t > s || (t == s && q < lane)) ? 1u : 0u;
        }
    }
    __syncthreads();
    if (lane < n) T.sc[r] = (uint16_t)s, T.ord[r] = (uint8_t)o;
    __syncthreads();
}

__global__ __launch_bounds__(64) void lq_rank_kernel(RegionDev *__restrict__ regions, const char *__restrict__ strpool,
                                                      unsigned long long cap, uint32_t min_n) {
    __shared__ RankLds T;
    static_assert(kRankKm == 32, "a position's k-mers are one half wavefront");
    RegionDev &G = regions[blockIdx.x];
    const int lane = (int)threadIdx.x;
    const uint32_t n_ok = G.n_ok;
    if (!G.want_rank || n_ok < min_n || n_ok < 1u || n_ok > (uint32_t)kRankMax) return;   // (ranked stays 0)
    const int n = (int)n_ok;
    uint32_t off = 0, len = 0;
    if (lane < n) off = G.cand_off[lane], len = G.cand_len[lane];
    if (__ballot((unsigned long long)off + len > cap) != 0ull) return;   // the pool was too small: this launch is repeated
    if (lane < n) T.off[lane] = off, T.len[lane] = (uint16_t)len, T.ord[lane] = (uint8_t)lane;
    __syncthreads();
    const unsigned char *pool = (const unsigned char *)strpool;
    rank_stage(T, pool, n, 0, lane);
    rank_pass(T, n, 1, lane);
    rank_sort(T, n, lane);
    rank_pass(T, n, kRankTop, lane);
    const uint32_t kmaxlen = T.len[T.ord[0]], kmaxscore = T.sc[0];
    const bool tail = kmaxlen > 500u || (kmaxlen > 200u && kmaxscore < 200u);
    if (tail) {
        __syncthreads();
        if (lane >= 1 && lane < n && T.ord[lane] == 0u) {   // find_ref_lqseq: input 0 to the front, a swap
            const uint16_t s0 = T.sc[0];
            T.ord[lane] = T.ord[0], T.sc[0] = T.sc[lane], T.sc[lane] = s0, T.ord[0] = 0u;
        }
        __syncthreads();
        if (lane < n) T.saved[T.ord[lane]] = T.sc[lane];
        rank_stage(T, pool, n, 1, lane);
        rank_pass(T, n, 1, lane);
        rank_sort(T, n, lane);
        rank_pass(T, n, kRankTop, lane);
        if (lane < n) T.sc[lane] = (uint16_t)(T.sc[lane] + T.saved[T.ord[lane]]);
        __syncthreads();
    }
    rank_sort(T, n, lane);
    if (lane < n) G.rank_order[lane] = T.ord[lane], G.rank_kscore[lane] = T.sc[lane];
    if (lane == 0) G.rank_tail = tail ? 1u : 0u, G.ranked = 1u;
}

// ---------------------------------------------------------------------------------------------------------------------------
// K22: the phasing and ranking of a HiFi pile's candidates (nd_phase.h: hifi_phase_host; lib/nextcorrect.c:512-737, 787-948), behind
// K11 on the strings K11 left in the pool (or on the pool of a batch of piles: DeviceAligner::run_phase).
//
// hifi_phase_kernel: one workgroup of four wavefronts per pile; a wavefront takes the regions w, w + 4, ...  The rule's steps over
// all regions of a pile are loops over the pile's regions between __syncthreads(): (1) classes, select_most2, the first pass over the
// heterozygous sites; (2) the second pass, where has_heter && !phase[0].s; (3) mark_del; (4) the compaction, the decision, the sort
// by length and the trims.  The pile's phase[] table lives in LDS, a word for s and a word for d (bit 31: del) per read, added to
// with LDS atomics -- sums, whatever the order; the reference's uint16_t is the low half of the word, so that it wraps as the
// reference's does.  A region's candidates sit one per lane, position j in lane j, as two words: A = input index | class << 8 |
// kscore << 16 and B = length | source read << 16; class = the smallest input index with the same string (exact: lanes over bytes
// hash every string, pairs of equal length and hash are compared byte by byte), and same_seq is a comparison of classes ever after.
// Swaps, the sort and the reversal are shuffles of the two words; the partition by swaps runs on wave-uniform scalars over the
// ballot of the flags, its pairs are disjoint.  Between the steps A waits in `work`, 40 words a region.  The strings are read again
// only by the three predicates of the second pass (uniform scalar loops) and by the ranking.  A region that reaches the ranking is
// left as kPhasePending for hifi_phase_rank_kernel.
// hifi_phase_rank_kernel: one wavefront per region, K14's method with c = 40: every sequence is counted, so a pass holds up to
// 40 x 32 distinct k-mers in a 2,048-slot table; the tail windows are staged over the head windows; the head scores are kept by
// source read (the last position of a read wins, as the reference's table indexed by read does).
constexpr int kPhThreads = 256, kPhWaves = kPhThreads / 64;
constexpr uint32_t kPhDel = 1u << 31;
constexpr uint8_t kPhWorking = 254;   // a region between the steps (kPhasePending: it waits for the ranking)
constexpr int kPhSlots = 2048;

struct PhaseLds {
    uint32_t s[kPhaseReads];   // [15:0]: phase[].s
    uint32_t d[kPhaseReads];   // [15:0]: phase[].d, bit 31: phase[].del
    uint32_t heter, err;
};

__device__ __forceinline__ uint32_t ph_sum(uint32_t v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}
__device__ __forceinline__ int ph_sum(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m);
    return v;
}

// class of the candidate in every lane < nc: the smallest input index with the same bytes
__device__ __forceinline__ uint32_t ph_classes(const unsigned char *__restrict__ pool, uint32_t off, uint32_t len, int nc, int lane) {
    uint32_t hash = 0;
    for (int i = 0; i < nc; i++) {
        const uint32_t oi = __shfl(off, i), li = __shfl(len, i);
        uint32_t h = 0;
        for (uint32_t b = (uint32_t)lane; b < li; b += 64u) h += ((uint32_t)pool[(size_t)oi + b] + 1u) * ((b * 0x9e3779b1u) | 1u);
        h = ph_sum(h);
        if (lane == i) hash = h;
    }
    uint32_t cls = (uint32_t)lane;
    bool found = false;
    for (int j = 0; j < nc; j++) {   // the classes' first members, ascending
        const uint32_t oj = __shfl(off, j), lj = __shfl(len, j), hj = __shfl(hash, j), cj = __shfl(cls, j);
        if (cj != (uint32_t)j) continue;
        unsigned long long m = __ballot(lane > j && lane < nc && !found && len == lj && hash == hj);
        for (int t = 0; t < 64 && m != 0ull; t++) {
            const int i = __ffsll((long long)m) - 1;
            m &= m - 1ull;
            const uint32_t oi = __shfl(off, i);
            uint32_t diff = 0;
            for (uint32_t b = (uint32_t)lane; b < lj; b += 64u) diff |= (uint32_t)(pool[(size_t)oi + b] ^ pool[(size_t)oj + b]);
            if (__ballot(diff != 0u) == 0ull && lane == i) cls = (uint32_t)j, found = true;
        }
    }
    return cls;
}

// the election of select_most2_lqseq / select_most2_lqseq_with_kscore over the eligible positions of [0, n)
__device__ __forceinline__ int ph_elect(uint32_t A, uint32_t B, unsigned long long elig, int n) {   // m1 | m2 << 8
    int m1 = 0, m2 = 0;
    uint32_t ks1 = __shfl(A, 0) >> 16, or1 = __shfl(B, 0) >> 16, ks2 = ks1;
    for (int j = 0; j < n; j++) {
        const uint32_t ksj = __shfl(A, j) >> 16, orj = __shfl(B, j) >> 16;
        if (!((elig >> j) & 1ull)) continue;
        if (ksj > ks1 || (ksj == ks1 && orj < or1)) {
            m2 = m1, ks2 = ks1;
            m1 = j, ks1 = ksj, or1 = orj;
        } else if (m2 == m1 || ksj > ks2) {
            m2 = j, ks2 = ksj;
        }
    }
    return m1 | m2 << 8;
}

// select_most2_lqseq: a class's first position of [0, n) takes the class's size there, every other position 1
__device__ __forceinline__ int ph_most2(uint32_t &A, uint32_t B, int n, int lane) {
    const uint32_t cls = (A >> 8) & 0xffu;
    uint32_t size = 0;
    bool first = true;
    for (int q = 0; q < n; q++) {
        const uint32_t cq = (__shfl(A, q) >> 8) & 0xffu;
        if (cq == cls) {
            size++;
            if (q < lane) first = false;
        }
    }
    if (lane < n) A = (A & 0xffffu) | (first ? size : 1u) << 16;
    return ph_elect(A, B, __ballot(lane < n && first), n);
}

// the partition by swaps (lib/nextcorrect.c:524-537, 599-609) over the flags D of [0, n): returns the new length
__device__ __forceinline__ int ph_partition(uint32_t &A, uint32_t &B, unsigned long long D, int n, int lane) {
    int k = n, partner = lane;
    for (int j = 0; j < n && j < k; j++) {
        if (!((D >> j) & 1ull)) continue;
        for (k--; k > j; k--)
            if (!((D >> k) & 1ull)) {
                if (lane == j) partner = k;
                if (lane == k) partner = j;
                break;
            }
    }
    A = __shfl(A, partner), B = __shfl(B, partner);
    return k;
}

// remove_differ_len_lqseq (:512-539)
__device__ __forceinline__ int ph_differ_len(uint32_t &A, uint32_t &B, int &n, int span, int lane) {
    const int a = span / 10 > 30 ? span / 10 : 30, offset = a < span / 3 ? a : span / 3;
    const int len = (int)(B & 0xffffu);
    const bool ok = len + offset >= span && len <= span + offset;
    const unsigned long long in = __ballot(lane < n), okm = __ballot(lane < n && ok);
    const int s = __popcll(okm);
    if (s != n && (s >= n / 2 || (s >= n / 3 && s >= 3))) n = ph_partition(A, B, in & ~okm, n, lane);
    return s;
}

// the three predicates of the second pass: wave-uniform scalar loops over the pool's bytes
__device__ __forceinline__ int ph_prefixhomo(const unsigned char *a, int na, const unsigned char *b, int nb) {
    int i = 0, j = 0;
    while (i < na && j < nb) {
        if (a[i] != b[j]) return 0;
        while (i + 1 < na && a[i] == a[i + 1]) i++;
        while (j + 1 < nb && b[j] == b[j + 1]) j++;
        i++, j++;
    }
    return 1;
}
__device__ __forceinline__ void ph_run_ends(const unsigned char *q, int n, int &s, int &e) {
    s = 0;
    while (s + 1 < n && q[s] == q[s + 1]) s++;
    e = n - 1;
    while (e > 0 && q[e - 1] == q[e]) e--;
}
__device__ __forceinline__ int ph_homo_end(const unsigned char *a, int na, const unsigned char *b, int nb) {
    int as, ae, bs, be;
    ph_run_ends(a, na, as, ae);
    ph_run_ends(b, nb, bs, be);
    if (ae <= as && be <= bs) return 1;
    if (ae - as != be - bs) return 0;
    for (int i = 0; i <= ae - as; i++)
        if (a[i + as] != b[i + bs]) return 0;
    return 1;
}
__device__ __forceinline__ int ph_trim_endssr(const unsigned char *a, int na, const unsigned char *b, int nb) {
    if (na < nb) {
        const unsigned char *t = a;
        a = b, b = t;
        const int tn = na;
        na = nb, nb = tn;
    }
    int i;
    for (i = 0; i < nb; i++)
        if (a[i] != b[i]) return 0;
    for (int j = na - 1; j >= i; j--) {
        const int at = nb - (na - j);
        if (at < 0 || a[j] != b[at]) return 0;   // (in front of the shorter string: a mismatch, as in nd_phase.h)
    }
    return 1;
}
__device__ __forceinline__ int ph_like_first(const unsigned char *a, int na, const unsigned char *b, int nb) {
    return ph_homo_end(a, na, b, nb) || ph_trim_endssr(a, na, b, nb) || ph_prefixhomo(a, na, b, nb);
}

// a region's positions from `work` and its record of K11
__device__ __forceinline__ void ph_load(const RegionDev &G, const uint32_t *__restrict__ W, int nc, int lane, uint32_t &A, uint32_t &B,
                                        uint32_t &off) {
    A = 0u, B = 0u, off = 0u;
    if (lane < nc) {
        A = W[lane];
        const uint32_t i = A & 0xffu;
        B = (uint32_t)G.cand_len[i] | (uint32_t)G.cand_rank[i] << 16;
        off = G.cand_off[i];
    }
}
__device__ __forceinline__ void ph_finish(PhaseRegionDev &O, uint32_t A, int nc, int lane, uint8_t kind, int n, uint32_t lower,
                                          uint32_t seed, uint32_t seed_pos) {
    if (lane < kPhaseCanMax) {
        O.perm[lane] = lane < nc ? (uint8_t)(A & 0xffu) : (uint8_t)0;
        O.kscore[lane] = lane < nc ? (uint16_t)(A >> 16) : (uint16_t)0;
    }
    if (lane == 0) O.kind = kind, O.lower = (uint8_t)lower, O.tail = 0, O.n = (int16_t)n, O.seed = (uint8_t)seed, O.seed_pos = (uint8_t)seed_pos;
}

__global__ __launch_bounds__(kPhThreads) void hifi_phase_kernel(const RegionDev *__restrict__ regions, const char *__restrict__ strpool,
                                                                 unsigned long long cap, PhasePileDev *__restrict__ piles,
                                                                 PhaseRegionDev *__restrict__ out, uint32_t *__restrict__ work) {
    __shared__ PhaseLds L;
    PhasePileDev &P = piles[blockIdx.x];
    const int tid = (int)threadIdx.x, lane = tid & 63, w = tid >> 6;
    const uint32_t first = P.first_region, nreg = P.n_regions, n_aligned = P.n_aligned;
    {
        uint32_t e = P.decline ? kPhaseErrHook : 0u;
        if (n_aligned > kPhaseReads) e |= kPhaseErrReads;
        if (nreg > kPhaseRegionsMax) e |= kPhaseErrRegions;
        if (e) {   // (the whole workgroup)
            if (tid == 0) P.err = e, P.has_heter = 0u, P.pass2 = 0u;
            return;
        }
    }
    for (uint32_t i = (uint32_t)tid; i < n_aligned; i += (uint32_t)kPhThreads) L.s[i] = 0u, L.d[i] = 0u;
    if (tid == 0) L.heter = 0u, L.err = 0u;
    __syncthreads();
    const unsigned char *pool = (const unsigned char *)strpool;

    // (1) classes, select_most2, the heterozygous sites (:789-810)
    for (uint32_t r = (uint32_t)w; r < nreg; r += (uint32_t)kPhWaves) {
        const RegionDev &G = regions[first + r];
        PhaseRegionDev &O = out[first + r];
        uint32_t *W = work + (size_t)(first + r) * kPhaseWorkWords;
        const int nc = (int)G.n_ok;
        if (nc == 0) continue;   // (the record stays as the caller cleared it: kPhaseEmpty)
        if (nc > kPhaseCanMax) {
            if (lane == 0) atomicOr(&L.err, kPhaseErrPool);
            continue;
        }
        uint32_t off = 0, len = 0, src = 0;
        if (lane < nc) off = G.cand_off[lane], len = G.cand_len[lane], src = G.cand_rank[lane];
        const bool bad_pool = __ballot(lane < nc && (unsigned long long)off + len > cap) != 0ull;
        const bool bad_src = __ballot(lane < nc && src >= n_aligned) != 0ull;
        if (bad_pool || bad_src) {
            if (lane == 0) atomicOr(&L.err, (bad_pool ? kPhaseErrPool : 0u) | (bad_src ? kPhaseErrSource : 0u));
            continue;
        }
        uint32_t A = (uint32_t)lane | ph_classes(pool, off, len, nc, lane) << 8;
        if (lane >= nc) A = 0u;
        const uint32_t B = len | src << 16;
        const int sk = ph_most2(A, B, nc, lane), s = sk & 0xff, k = sk >> 8;
        const uint32_t As = __shfl(A, s), Ak = __shfl(A, k), Bs = __shfl(B, s), Bk = __shfl(B, k);
        const uint32_t os = __shfl(off, s), ok = __shfl(off, k);
        const uint32_t kss = As >> 16, ksk = Ak >> 16, ls = Bs & 0xffffu, lk = Bk & 0xffffu;
        uint32_t indexs = 0;
        if (s != k && ksk >= 3u && ls == lk) {
            if (s == 0 || k == 0) {
                const uint32_t c0 = ((s == 0 ? As : Ak) >> 8) & 0xffu, ch = ((s == 0 ? Ak : As) >> 8) & 0xffu, c = (A >> 8) & 0xffu;
                if (lane < nc) {
                    if (c == c0) atomicAdd(&L.s[src], 1u);
                    else if (c == ch) atomicAdd(&L.d[src], 1u);
                }
            }
            indexs = 1;
        }
        bool het = indexs == 1u;
        if (!het && s != k && ksk >= 5u && (double)(int)(kss + ksk) >= (double)nc * 0.8)
            het = !ph_prefixhomo(pool + os, (int)ls, pool + ok, (int)lk);
        if (het && lane == 0) atomicOr(&L.heter, 1u);
        if (lane < (int)kPhaseWorkWords) W[lane] = A;
        if (lane == 0) O.kind = kPhWorking, O.indexs = (uint8_t)indexs, O.n = (int16_t)nc;
    }
    __syncthreads();
    const uint32_t err = L.err, heter = L.heter;
    const bool pass2 = heter != 0u && (L.s[0] & 0xffffu) == 0u;
    __syncthreads();   // (phase[0].s is read before the second pass adds to it)
    if (err) {
        if (tid == 0) P.err = err, P.has_heter = 0u, P.pass2 = 0u;
        return;
    }
    if (tid == 0) P.err = 0u, P.has_heter = heter, P.pass2 = pass2 ? 1u : 0u;

    // (2) no SNP was found, but a candidate site (:812-854)
    if (pass2)
        for (uint32_t r = (uint32_t)w; r < nreg; r += (uint32_t)kPhWaves) {
            const RegionDev &G = regions[first + r];
            PhaseRegionDev &O = out[first + r];
            const int nc = (int)G.n_ok;
            if (nc == 0) continue;
            uint32_t A, B, off;
            ph_load(G, work + (size_t)(first + r) * kPhaseWorkWords, nc, lane, A, B, off);
            const int sk = ph_elect(A, B, ~0ull, nc), s = sk & 0xff, k = sk >> 8;
            const uint32_t As = __shfl(A, s), Ak = __shfl(A, k), Bs = __shfl(B, s), Bk = __shfl(B, k), B0 = __shfl(B, 0);
            const unsigned char *ps = pool + __shfl(off, s), *pk = pool + __shfl(off, k), *p0 = pool + __shfl(off, 0);
            const int kss = (int)(As >> 16), ksk = (int)(Ak >> 16), ls = (int)(Bs & 0xffffu), lk = (int)(Bk & 0xffffu), l0 = (int)(B0 & 0xffffu);
            if (s != k && ksk >= 5 && (double)(kss + ksk) >= (double)nc * 0.8 &&
                (ls >= lk + 5 || lk >= ls + 5 || !ph_prefixhomo(ps, ls, pk, lk))) {
                int s_, k_;
                if (s == 0) s_ = 1, k_ = 0;
                else if (k == 0) s_ = 0, k_ = 1;
                else s_ = ph_like_first(ps, ls, p0, l0), k_ = ph_like_first(pk, lk, p0, l0);
                if ((s_ != 0) != (k_ != 0)) {
                    const uint32_t cs = ((s_ ? As : Ak) >> 8) & 0xffu, ch = ((s_ ? Ak : As) >> 8) & 0xffu, c = (A >> 8) & 0xffu;
                    if (lane < nc) {
                        if (c == cs) atomicAdd(&L.s[B >> 16], 1u);
                        else if (c == ch) atomicAdd(&L.d[B >> 16], 1u);
                    }
                    if (lane == 0) O.indexs = 2;
                }   // (else: indexs stays)
            } else if (lane == 0) O.indexs = 0;
        }
    __syncthreads();

    // (3) mark_del_lqseq (:570-588)
    for (uint32_t r = (uint32_t)w; r < nreg; r += (uint32_t)kPhWaves) {
        const RegionDev &G = regions[first + r];
        const int nc = (int)G.n_ok;
        if (nc == 0) continue;
        uint32_t A, B, off;
        ph_load(G, work + (size_t)(first + r) * kPhaseWorkWords, nc, lane, A, B, off);
        const uint32_t src = B >> 16, s16 = L.s[src] & 0xffffu, d16 = L.d[src] & 0xffffu;
        const int kk = __popcll(__ballot(lane >= 1 && lane < nc && s16 >= 3u && d16 == 0u));
        if (lane < nc && (kk >= 2 ? d16 != 0u : (s16 < d16 || d16 >= 3u))) atomicOr(&L.d[src], kPhDel);
    }
    __syncthreads();

    // (4) remove_differ_phase_lqseq (:590-610) and a region's turn up to its ranking (:874-933)
    for (uint32_t r = (uint32_t)w; r < nreg; r += (uint32_t)kPhWaves) {
        const RegionDev &G = regions[first + r];
        PhaseRegionDev &O = out[first + r];
        uint32_t *W = work + (size_t)(first + r) * kPhaseWorkWords;
        const int nc = (int)G.n_ok;
        if (nc == 0) continue;
        uint32_t A, B, off;
        ph_load(G, W, nc, lane, A, B, off);
        int n = ph_partition(A, B, __ballot(lane < nc && (L.d[B >> 16] & kPhDel) != 0u), nc, lane);
        if (n == 0) {   // every candidate's read was phased away
            ph_finish(O, A, nc, lane, kPhaseDropped, 0, 0u, 0u, 0u);
            continue;
        }
        const uint32_t indexs = O.indexs;
        const int span = (int)(G.end - G.start + 1u);
        const int sk = ph_most2(A, B, n, lane);
        int s = sk & 0xff, k = sk >> 8;
        {
            const uint32_t As = __shfl(A, s), Ak = __shfl(A, k), Bs = __shfl(B, s), B0 = __shfl(B, 0);
            const int kss = (int)(As >> 16), ksk = (int)(Ak >> 16);
            const int ps = (int)(L.s[Bs >> 16] & 0xffffu), pd = (int)(L.d[Bs >> 16] & 0xffffu);
            const int my_s = (int)(L.s[B >> 16] & 0xffffu), my_d = (int)(L.d[B >> 16] & 0xffffu);
            if (indexs && s != k && s != 0 && ksk >= 3 && ps >= pd + 3) {
                const uint32_t cs = (As >> 8) & 0xffu, ck = (Ak >> 8) & 0xffu, c = (A >> 8) & 0xffu;
                const bool act = lane >= 1 && lane < n && my_d < 3;
                const int sp = ph_sum(act && c == cs ? my_s - my_d : 0), kp = ph_sum(act && c != cs && c == ck ? my_s - my_d : 0);
                if (sp < kp) s = k;
            } else if ((int)(B0 & 0xffffu) > 50 && kss < n / 3 && kss < 3) {
                const int sl = ph_differ_len(A, B, n, span, lane);
                if (sl <= 3) {   // large length SD: the seed's own version
                    s = 0;
                    if (lane == 0) A = (A & 0xffffu) | 65534u << 16;
                }
            }
        }
        const uint32_t Af = __shfl(A, s);
        const int ksf = (int)(Af >> 16);
        if (ksf > 2 || ksf >= n / 2) {
            ph_finish(O, A, nc, lane, kPhaseSeed, -2, ksf < n / 2 ? 1u : 0u, Af & 0xffu, (uint32_t)s);
            continue;
        }
        ph_differ_len(A, B, n, span, lane);
        bool dropped = false;
        if (n > 4) {
            {   // qsort(compare_seq_by_len), stable: a rank by counting, then the inverse by search
                const uint32_t len = B & 0xffffu;
                int rk = lane < n ? 0 : lane;
                for (int q = 0; q < n; q++) {
                    const uint32_t lq = __shfl(B, q) & 0xffffu;
                    if (lane < n && (lq < len || (lq == len && q < lane))) rk++;
                }
                int from = lane;
                for (int q = 0; q < n; q++)
                    if (__shfl(rk, q) == lane) from = q;
                A = __shfl(A, from), B = __shfl(B, from);
            }
            k = n / 2;
            for (int t = 0; t < kPhaseCanMax && n > k; t++) {
                const int l1 = (int)(__shfl(B, n - 1) & 0xffffu), lk = (int)(__shfl(B, k) & 0xffffu), l2 = (int)(__shfl(B, n - 2) & 0xffffu);
                if (!(l1 > 2 * lk || (double)l1 >= 1.4 * (double)l2)) break;
                n--;
            }
            if (k == n) dropped = true;
            else {
                k = n / 2;
                if ((int)(__shfl(B, 0) & 0xffffu) < (int)(__shfl(B, k) & 0xffffu) / 2) {
                    const int from = lane < n ? n - 1 - lane : lane;   // reverse_lqseq
                    A = __shfl(A, from), B = __shfl(B, from);
                    for (int t = 0; t < kPhaseCanMax && n > 1; t++) {
                        if (!((int)(__shfl(B, n - 1) & 0xffffu) < (int)(__shfl(B, k) & 0xffffu) / 2)) break;
                        n--;
                    }
                    if (k == n) dropped = true;
                }
            }
        }
        if (dropped) {
            ph_finish(O, A, nc, lane, kPhaseDropped, 0, 0u, 0u, 0u);
            continue;
        }
        if (lane < (int)kPhaseWorkWords) W[lane] = A;
        if (lane == 0) O.n = (int16_t)n, O.kind = kPhasePending;
    }
}

struct PhRankLds {
    uint32_t tab[kPhSlots];                // [31:16] k-mer, [15:0] count; 0: empty
    uint32_t off[kRankMax];                // input order: pool offset, length, source read
    uint16_t len[kRankMax], src[kRankMax];
    uint16_t km[kRankMax * kRankKm];       // input order: the staged window's k-mers
    uint16_t sc[kRankMax], saved[kRankMax];  // by position
    uint8_t code[kRankMax * kRankWin];     // input order: the staged window's byte codes
    uint8_t ord[kRankMax];                 // position -> input index
};
__device__ __forceinline__ uint32_t ph_slot(uint32_t km) { return (km * 0x9e3bu >> 3) & (uint32_t)(kPhSlots - 1); }

// the window's k-mers of every sequence, input order (K14: rank_stage)
__device__ __forceinline__ void ph_stage(PhRankLds &T, const unsigned char *__restrict__ pool, int nc, int from_tail, int lane) {
    for (int i = lane; i < nc * kRankWin; i += 64) {
        const int s = i / kRankWin, b = i - s * kRankWin, len = (int)T.len[s];
        const int o = from_tail && len > kRankWin ? len - kRankWin : 0;
        T.code[i] = b < len ? (uint8_t)rank_code(pool[(size_t)T.off[s] + (size_t)(o + b)]) : (uint8_t)0;
    }
    __syncthreads();
    for (int i = lane; i < nc * kRankKm; i += 64) {
        const int s = i / kRankKm, k = i - s * kRankKm;
        uint32_t km = 0;
        if (k < rank_nkm((int)T.len[s])) {
            const uint8_t *c = &T.code[s * kRankWin + k];
#pragma unroll
            for (int x = 0; x < kRankK; x++) km = km << 2 | c[x];
        }
        T.km[i] = (uint16_t)km;
    }
    __syncthreads();
}

// count the k-mers of the positions [0, n), score every one of them (K14: rank_pass with c >= n)
__device__ __forceinline__ void ph_pass(PhRankLds &T, int n, int lane) {
    for (int i = lane; i < kPhSlots; i += 64) T.tab[i] = 0u;
    __syncthreads();
    for (int i = lane; i < n * kRankKm; i += 64) {
        const int p = i / kRankKm, k = i - p * kRankKm, s = (int)T.ord[p];
        if (k >= rank_nkm((int)T.len[s])) continue;
        const uint32_t km = T.km[s * kRankKm + k];
        uint32_t h = ph_slot(km);
        for (int t = 0; t < kPhSlots; t++, h = (h + 1u) & (uint32_t)(kPhSlots - 1)) {   // (<= 1,280 keys in 2,048 slots: an empty one exists)
            uint32_t cur = T.tab[h];
            if (cur == 0u) {
                cur = atomicCAS(&T.tab[h], 0u, km << 16 | 1u);
                if (cur == 0u) break;
            }
            if ((cur >> 16) == km) {
                atomicAdd(&T.tab[h], 1u);
                break;
            }
        }
    }
    __syncthreads();
    for (int i0 = 0; i0 < n * kRankKm; i0 += 64) {   // a position per half wavefront, a k-mer per lane of it
        const int i = i0 + lane, p = i / kRankKm, k = i - p * kRankKm;
        uint32_t v = 0;
        if (p < n) {
            const int s = (int)T.ord[p];
            if (k < rank_nkm((int)T.len[s])) {
                const uint32_t km = T.km[s * kRankKm + k];
                uint32_t h = ph_slot(km);
                for (int t = 0; t < kPhSlots; t++, h = (h + 1u) & (uint32_t)(kPhSlots - 1)) {
                    const uint32_t cur = T.tab[h];
                    if (cur == 0u) break;
                    if ((cur >> 16) == km) {
                        v = cur & 0xffffu;
                        break;
                    }
                }
            }
        }
#pragma unroll
        for (int m = kRankKm / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
        if (p < n && k == 0) T.sc[p] = (uint16_t)v;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void hifi_phase_rank_kernel(const RegionDev *__restrict__ regions, const char *__restrict__ strpool,
                                                              PhaseRegionDev *__restrict__ out, const uint32_t *__restrict__ work) {
    __shared__ PhRankLds T;
    static_assert(kRankKm == 32 && kRankMax == kPhaseCanMax, "a position's k-mers are one half wavefront");
    PhaseRegionDev &O = out[blockIdx.x];
    if (O.kind != kPhasePending) return;   // (the whole wavefront)
    const RegionDev &G = regions[blockIdx.x];
    const int lane = (int)threadIdx.x, nc = (int)G.n_ok, n = (int)O.n;
    if (nc < 1 || nc > kRankMax || n < 1 || n > nc) return;   // (cannot happen: hifi_phase_kernel left the region)
    const uint32_t A = lane < nc ? work[(size_t)blockIdx.x * kPhaseWorkWords + (uint32_t)lane] : 0u;
    if (lane < nc) T.off[lane] = G.cand_off[lane], T.len[lane] = G.cand_len[lane], T.src[lane] = G.cand_rank[lane];
    if (lane < n) T.ord[lane] = (uint8_t)(A & 0xffu);
    __syncthreads();
    const unsigned char *pool = (const unsigned char *)strpool;
    ph_stage(T, pool, nc, 0, lane);
    ph_pass(T, n, lane);
    const bool tail = T.len[T.ord[0]] > 100u;
    if (tail) {
        if (lane < n) {   // save_kscore by source read: the last position of a read wins
            uint16_t v = T.sc[lane];
            const uint16_t src = T.src[T.ord[lane]];
            for (int q = lane + 1; q < n; q++)
                if (T.src[T.ord[q]] == src) v = T.sc[q];
            T.saved[lane] = v;
        }
        ph_stage(T, pool, nc, 1, lane);
        ph_pass(T, n, lane);
        if (lane < n) T.sc[lane] = (uint16_t)(T.sc[lane] + T.saved[lane]);
        __syncthreads();
    }
    {   // qsort(compare_seq_by_kscore), stable, descending: a rank by counting
        uint32_t s = 0, o = 0, r = 0;
        if (lane < n) {
            s = T.sc[lane], o = T.ord[lane];
            for (int q = 0; q < n; q++) {
                const uint32_t t = T.sc[q];
                r += (t > s || (t == s && q < lane)) ? 1u : 0u;
            }
        }
        __syncthreads();
        if (lane < n) T.sc[r] = (uint16_t)s, T.ord[r] = (uint8_t)o;
        __syncthreads();
    }
    if (lane < kPhaseCanMax) {
        O.perm[lane] = lane < n ? T.ord[lane] : lane < nc ? (uint8_t)(A & 0xffu) : (uint8_t)0;
        O.kscore[lane] = lane < n ? T.sc[lane] : lane < nc ? (uint16_t)(A >> 16) : (uint16_t)0;
    }
    if (lane == 0) O.kind = kPhaseRanked, O.lower = 0, O.tail = tail ? 1 : 0, O.seed = 0, O.seed_pos = 0;
}

}  // namespace

void launch_lq_msa(LqPileDev *piles, LqJobDev *jobs, const LqPieceDev *pieces, const AlnTask *tasks, const AlnOut *outs, const uint32_t *ops,
                   const uint32_t *pool, uint64_t *hdr, uint32_t *lnk, uint32_t *cell_rec, int32_t *bnd, char *tmp_chars, char *out_chars,
                   int n_piles, int n_jobs, uint32_t warm, uint32_t force_repair, void *stream) {
    if (n_piles <= 0) return;
    hipStream_t st = (hipStream_t)stream;
    if (n_jobs > 0) {
        hipLaunchKernelGGL(lq_links_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, jobs, piles, pieces, tasks, outs, ops, pool, hdr, lnk);
        hipLaunchKernelGGL(lq_score_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, piles, jobs, hdr, lnk, cell_rec, bnd, warm ? warm : 1u);
    }
    hipLaunchKernelGGL(lq_stitch_kernel, dim3((unsigned)n_piles), dim3(64), 0, st, piles, jobs, hdr, lnk, cell_rec, bnd, force_repair);
    if (n_jobs > 0) hipLaunchKernelGGL(lq_walk_kernel, dim3((unsigned)n_jobs), dim3(64), 0, st, piles, jobs, cell_rec, tmp_chars);
    hipLaunchKernelGGL(lq_gather_kernel, dim3((unsigned)n_piles), dim3(64), 0, st, piles, jobs, tmp_chars, out_chars);
}


void launch_poa_align(PoaJobDev *jobs, const uint32_t *ids_wave, int n_wave, const uint32_t *ids_group, int n_group, const char *qpool,
                      const PoaRowDev *rows, const uint16_t *preds, int32_t *S, uint16_t *F, uint32_t *route, void *stream) {
    hipStream_t st = (hipStream_t)stream;
    if (n_wave > 0)
        hipLaunchKernelGGL(poa_align_kernel<1>, dim3((unsigned)n_wave), dim3(64), 0, st, jobs, ids_wave, qpool, rows, preds, S, F, route);
    if (n_group > 0)
        hipLaunchKernelGGL(poa_align_kernel<kPoaGroupWaves>, dim3((unsigned)n_group), dim3(kPoaGroupWaves * 64), 0, st, jobs, ids_group, qpool,
                           rows, preds, S, F, route);
}

void launch_poa_graph_start(PoaGraphDev *graphs, PoaXeDev *xe, unsigned char *arena, const char *seqs, const PoaSeqDev *seq_tab, int n,
                            void *stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(poa_graph_start, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, graphs, xe, arena, seqs, seq_tab);
}

void launch_poa_graph_rows(PoaGraphDev *graphs, const PoaRoundDev *round, int n_round, uint32_t r, unsigned char *arena,
                           const PoaSeqDev *seq_tab, PoaJobDev *jobs, void *stream) {
    if (n_round <= 0) return;
    hipLaunchKernelGGL(poa_graph_rows, dim3((unsigned)n_round), dim3(64), 0, (hipStream_t)stream, graphs, round, r, arena, seq_tab, jobs);
}

void launch_poa_graph_thread(PoaGraphDev *graphs, PoaXeDev *xe, const PoaRoundDev *round, int n_round, uint32_t r, unsigned char *arena,
                             const char *seqs, const PoaSeqDev *seq_tab, const PoaJobDev *jobs, void *stream) {
    if (n_round <= 0) return;
    hipLaunchKernelGGL(poa_graph_thread, dim3((unsigned)n_round), dim3(64), 0, (hipStream_t)stream, graphs, xe, round, r, arena, seqs, seq_tab,
                       jobs);
}

void launch_poa_graph_consensus(PoaGraphDev *graphs, const uint32_t *ids, int n, unsigned char *arena, char *out, uint32_t *out_len,
                                void *stream) {
    if (n <= 0) return;
    hipLaunchKernelGGL(poa_graph_consensus, dim3((unsigned)n), dim3(64), 0, (hipStream_t)stream, graphs, ids, arena, out, out_len);
}

void launch_lq_rank(RegionDev *regions, const char *strpool, unsigned long long strpool_cap, uint32_t min_n, int n_regions, void *stream) {
    if (n_regions <= 0) return;
    hipLaunchKernelGGL(lq_rank_kernel, dim3((unsigned)n_regions), dim3(64), 0, (hipStream_t)stream, regions, strpool, strpool_cap, min_n);
}

void launch_hifi_phase(const RegionDev *regions, const char *strpool, unsigned long long strpool_cap, PhasePileDev *piles, int n_piles,
                       PhaseRegionDev *out, uint32_t *work, int n_regions, void *stream) {
    if (n_piles <= 0 || n_regions <= 0) return;
    hipLaunchKernelGGL(hifi_phase_kernel, dim3((unsigned)n_piles), dim3(kPhThreads), 0, (hipStream_t)stream, regions, strpool, strpool_cap,
                       piles, out, work);
    hipLaunchKernelGGL(hifi_phase_rank_kernel, dim3((unsigned)n_regions), dim3(64), 0, (hipStream_t)stream, regions, strpool, out, work);
}

}  // namespace ndgpu
