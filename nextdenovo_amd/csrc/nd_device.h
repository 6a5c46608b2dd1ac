// Device-side task/record layouts shared by the HIP kernels and the host runtime.
#pragma once

#include <cstdint>

#include "nd_lockstep.h"
#include "nd_phase.h"

namespace ndgpu {

// Sequences live in one pool of 2-bit codes, 16 bases per uint32, base i of a word
// at bits [2i, 2i+1] (LSB first, so that the first mismatch of a snake is a
// count-trailing-zeros of the XOR).  Offsets are in BASES, so a target window
// may start anywhere inside a seed without re-packing.
struct AlnTask {
    uint64_t q_off;      // first query base in the pool
    uint64_t t_off;      // first target base in the pool
    int32_t q_len;
    int32_t t_len;
    int32_t max_d;       // edit budget  (lib/align.c:567,575)
    int32_t band;        // band cap     (lib/align.c:568,576)
    uint64_t trace_off;  // uint64-word offset of the task's trace (register path: a stream of <= 2 * max_d words;
                         // wide path: row d at trace_off + d*row_words)
    uint64_t mink_off;   // wide path: index of row 0 in the per-row min_k array; register path with checkpoints (segmented
                         // traceback): the task's first checkpoint slot
    uint64_t ops_off;    // first ops word of this task (uint32 units)
    uint32_t ops_cap;    // capacity in columns (= q_len + t_len)
    uint32_t row_words;  // wide path only: uint64 words per trace row
    uint64_t v_off;      // wide path only: first int of this task's global V scratch
    uint32_t v_mask;     // wide path only: V ring size - 1 (power of two - 1)
    uint32_t seg_off;    // segmented traceback: the task's first walker slot (TbSeg / TbSegOut)
};

enum : int32_t {
    ST_NONE = 0,       // band cap or edit budget exhausted: no alignment
    ST_FINISHED = 1,   // forward sweep reached (q_len, t_len)
    ST_ALIGNED = 2,    // traceback done, ops valid
    ST_GAP_ABORT = 3,  // > 250 consecutive gap columns in traceback (lib/align.c:542-545)
    ST_NEED_WIDE = 4,  // live band exceeded the LDS fast path; rerun in the wide kernel
};

struct AlnOut {
    int32_t status;
    int32_t d_final;
    int32_t k_final;
    int32_t x_final;   // aln_q_len
    int32_t y_final;   // aln_t_len
    int32_t n_cols;    // alignment columns; ops occupy columns [ops_cap - n_cols, ops_cap)
    int32_t d_steps;   // counters for the roofline accounting
    int32_t max_band;
    int64_t cells;
    uint32_t trace_end;  // register path: words of trace stream written (the finishing step's record ends here)
    int32_t fin_idx;     // register path: bits [7:0] cell index of k_final in the finishing step; bits [15:8] (checkpointing
                         // forward kernel) cell index, in the last checkpoint row, of the cell the finishing cell descends from
};

// ---- segmented traceback (K8a in pieces; ond_kernels.hip) ----
// The forward kernel leaves a checkpoint every 2^cshift edit steps: per cell of that row its furthest-reaching x and the cell of
// the checkpoint row before that its move bits lead back to (packed: x in [23:0], cell in [31:24]; 128 cells a slot), per row the
// trace position behind its record and its min_k.  A chase along those cells names, for every checkpoint row under the finishing
// step, the cell the traceback passes through; one WALKER per checkpoint then walks its stretch of rows on a lane of its own.
struct TbSeg {            // a walker: starts at the top of row d_top, owns (emits) rows d_own .. d_end
    int32_t task;         // index into the launch's task table; -1: unused slot
    int32_t d_top;        // first row walked (a checkpoint row, or the finishing step for a task's first walker)
    int32_t d_own;        // first row owned: d_top for the first walker, d_top - warm otherwise (the rows above it are walked
                          // without output: the walk's x falls in with the true walk's within a few rows, see tb_walk_kernel)
    int32_t d_end;        // last row owned
    int32_t x;            // the state at the top of row d_top: query position, cell index, the row's min_k, trace position
    int32_t idx;
    int32_t min_k;
    uint32_t pos;
};
struct TbSegOut {
    int32_t x_own, k_own; // the walk's state at the top of row d_own ...
    int32_t x_end, k_end; // ... and at the top of row d_end - 1 (what the next walker's x_own / k_own must equal)
    int32_t lead, trail;  // gap columns before the first match run of the owned rows / behind the last (lib/align.c:542-545 counts
                          // across walkers: the stitch carries them)
    uint32_t rows;        // owned rows walked
    uint32_t flags;       // kTbReset | kTbAbort | kTbTerminal | kTbBad
};
enum : uint32_t {
    kTbReset = 1,         // a match run inside the owned rows (the gap counter restarted)
    kTbAbort = 2,         // more than 250 gap columns in a row inside the owned rows
    kTbTerminal = 4,      // reached the alignment's start
    kTbBad = 8,           // the walk ended where it must not (in the warm-up rows): the task is walked again in one piece
};
constexpr int kCkptCells = 128;
constexpr int32_t kTbRefused = 1 << 16;   // AlnOut::fin_idx: the stitch refused the task (host statistics) ...
constexpr int32_t kTbSeen = 1 << 17;      // ... of the tasks it saw

// ---- main-phase consensus on the device (msa_kernels.hip) ---------------------------------
// Packed alignment tag (reference: align_tag, lib/nextcorrect.h:28-32): t_pos+1 in bits
// [31:11] (so the head sentinel t_pos=-1,delta=0,base=0 packs to 0), delta in [10:3]
// (an insertion run is at most 251 columns, lib/align.c:542), base code in [2:0]
// (A0 T1 G2 C3 -4, lib/nextcorrect.c:52-62).
constexpr uint32_t kTagHead = 0u;
__host__ __device__ inline uint32_t tag_pack(int32_t t_pos, uint32_t delta, uint32_t base) {
    return ((uint32_t)(t_pos + 1) << 11) | (delta << 3) | base;
}
__host__ __device__ inline int32_t tag_tpos(uint32_t g) { return (int32_t)(g >> 11) - 1; }
__host__ __device__ inline uint32_t tag_delta(uint32_t g) { return (g >> 3) & 0xffu; }
__host__ __device__ inline uint32_t tag_base(uint32_t g) { return g & 7u; }

// The lanes whose predicate holds, as a mask.  __ballot() goes through an int (v_cndmask 0/1, v_cmp_ne); the builtin is the
// compare's own result.  The lane-by-lane interpreter of the kernel tests has __ballot only.
#if defined(SIMT_EMULATION)
inline unsigned long long wave_ballot(bool p) { return __ballot(p); }
#elif defined(__HIPCC__)
__device__ __forceinline__ unsigned long long wave_ballot(bool p) { return __builtin_amdgcn_ballot_w64(p); }
#endif

struct ReadDev {            // one per pile record (index 0 of a pile = the seed itself)
    int32_t task;           // index into the AlnTask/AlnOut tables, -1 for the seed
    uint32_t aln_start;     // inclusive seed window as handed to nextCorrect
    uint32_t aln_end;
    uint64_t tag_off;       // first tag slot of this read (uint32 units)
    uint64_t colidx_off;    // first column-index slot (uint32 units), capacity = window length
    // filled on the device
    uint32_t shift;         // first kept alignment column (get_align_shift)
    uint32_t aln_len;       // kept columns (0: dropped)
    uint32_t t_s, t_e;      // seed coordinates after trimming
    uint32_t q_start;       // query offset of column `shift`
    uint32_t accepted;      // passed min_len_aln and the coverage cut
    uint32_t pad_;
};

struct PileDev {
    uint32_t seed_len;
    uint32_t n_reads;       // records incl. the seed
    uint32_t first_read;    // index of the seed's ReadDev
    uint32_t min_len_aln;
    uint32_t max_cov_aln;
    int32_t factor;         // 3 (ont/clr) or 4 (hifi)   lib/nextcorrect.c:2147
    uint64_t seed_off;      // pool offset of the seed (bit 63: resident DB)
    uint64_t col_off;       // first slot of the per-column arrays (seed_len + 1 slots per pile)
    uint64_t acc_off;       // first slot of the accepted-read list (n_reads slots)
    // filled on the device
    uint32_t n_acc;         // accepted reads (incl. seed)
    uint32_t n_cells;       // 6 * sum(max_size)
    uint32_t n_tags;        // sum of kept columns = upper bound of link entries
    uint32_t path_len;
    // filled by the host between the two halves of the phase
    uint64_t cell_off;      // first cell of this pile
    uint64_t ent_off;       // first link entry of this pile
    uint64_t path_off;      // first path slot (capacity n_cells / 6)
    int32_t origin_t;       // backtrack origin written by the scoring kernel
    uint32_t origin_db;     // delta << 3 | base
    uint32_t err;           // nonzero: device-side capacity error
    uint32_t n_links;       // distinct (pp,ppp) links of the pile (written by the scoring kernel)
    // scoring segments (K10): filled by the host with the cell / link offsets
    uint32_t seg_off;       // index of the pile's first segment record
    uint32_t n_seg;
    uint32_t n_repair;      // segments the stitch kernel scored again (written by it)
    uint32_t tier;          // 1: scored with the large LDS tables (the column scan's verdict, fixed for the launch)
};

// ---- low-quality-region rounds (K12, lq_kernels.hip) ----
constexpr uint32_t kLqRoundRows = 30;  // rows of a round: the candidates the second MSA takes per region
struct LqPieceDev {          // one (row, region) slot of a pile's round, row-major (kLqRoundRows rows x n_regions)
    int32_t task;            // index into the round's AlnTask / AlnOut tables, -1: nothing aligned ('M' row)
    uint32_t sl;             // length of the region's pseudo-seed
};
struct LqPileDev {
    uint32_t first_piece, n_regions;
    uint32_t link_len;       // columns of the linked pseudo-seed: 1 + sum(sl + 1)
    int32_t factor;          // 2 (HiFi 4)     lib/nextcorrect.c:1262
    int32_t qv_factor;       // 5 (HiFi 2)     lib/nextcorrect.c:1303
    uint32_t row_cap;        // capacity in cell rows ((column, delta) pairs) of the pile's cell records
    uint32_t out_cap;        // capacity of the pile's output characters
    uint32_t first_job, n_jobs;  // the pile's jobs (K12a), in column order
    uint32_t n_repair;       // (written by the stitch) jobs it scored again from their predecessor's true scores
    uint64_t cell_off;       // first cell record (6 per cell row); cell_off / 6 = the pile's first scratch character
    uint64_t out_off;        // first output character
    // written by the kernels
    uint32_t out_len;
    uint32_t err;            // nonzero: declined (capacity, or an alignment that does not end at both sequence ends)
    uint32_t n_rows;         // cell rows of the pile
    uint32_t pad_;
};
struct LqJobDev {            // K12a's unit of work: regions [g_a, g_b) of a pile, each with the 'N' column in front of it
    uint32_t pile;
    uint32_t g_a, g_b;
    uint32_t t0, t1;         // columns [t0, t1) of the linked pseudo-seed (t0 = the 'N' in front of region g_a; the last job ends behind the closing 'N')
    uint32_t row_cap, lnk_cap;   // capacity of the job's streams: cell-row headers, link words
    uint32_t row0;           // (stitch) the job's first cell row within the pile
    uint64_t hdr_off, lnk_off;
    // written by K12a
    uint32_t n_rows, n_links, err;
    // written by K12b (scores): links of the boundary column it started from / of its last column, the smallest offset-carrying
    // candidate and the largest absolute value it compared (raw), a capacity error
    uint32_t score_err;
    uint32_t n_spec, n_fin;
    int32_t mn, mx;
    // written by K12d (walk)
    uint32_t out_len, walk_err, walk_end, pad_;
};
constexpr int kLqLinkCap = 384;      // links per column the scoring tables (and a job's boundary planes) hold
// K12: links per job (lq_links), scores + best links per job from a speculative start (lq_score), boundary checks / repairs per pile
// (lq_stitch), walk per job (lq_walk), the pile's characters (lq_gather).  bnd: 4 x kLqLinkCap words per job; tmp_chars: one per cell row.
void launch_lq_msa(LqPileDev *piles, LqJobDev *jobs, const LqPieceDev *pieces, const AlnTask *tasks, const AlnOut *outs, const uint32_t *ops,
                   const uint32_t *pool, uint64_t *hdr, uint32_t *lnk, uint32_t *cell_rec, int32_t *bnd, char *tmp_chars, char *out_chars,
                   int n_piles, int n_jobs, uint32_t warm, uint32_t force_repair, void *stream);

// ---- POA: one sequence against the graph (K13, lq_kernels.hip) ----
struct PoaRowDev {           // row i + 1 of a job = the i-th node of its graph in topological order
    uint32_t pred_off;       // first predecessor row (uint16 units, relative to the job's pred_off)
    uint16_t n_pred;         // >= 1: in-edge rows in insertion order, or row 0 alone
    uint8_t base;            // the node's byte
    uint8_t sink;            // the node has no out-edge
};
struct PoaJobDev {
    uint32_t X, Y;           // rows of the graph, bases of the query (1..65535, 1..9999)
    uint64_t q_off;          // first query byte
    uint64_t row_off;        // first PoaRowDev
    uint64_t pred_off;       // first predecessor entry
    uint64_t cell_off;       // first cell of the job's (X + 1)(Y + 1) scores / origins
    uint64_t route_off;      // first route word (capacity X + Y)
    uint32_t route_len;      // written by the kernel: steps of the walk back from the best sink
    uint32_t pad_;
};
constexpr int kPoaGroupWaves = 8;   // wavefronts of the workgroup form
constexpr uint32_t kPoaGroupMinLen = 1024;   // query bases from which the workgroup form takes a job (DESIGN.md section 0a'')
// ids_wave / ids_group: the jobs each form takes (device, n_wave / n_group indices into jobs)
void launch_poa_align(PoaJobDev *jobs, const uint32_t *ids_wave, int n_wave, const uint32_t *ids_group, int n_group, const char *qpool,
                      const PoaRowDev *rows, const uint16_t *preds, int32_t *S, uint16_t *F, uint32_t *route, void *stream);

// ---- POA: the graph itself on the device (K19, lq_kernels.hip; the arena's parts: poa_arena_layout of nd_lqplan.h) ----
struct PoaGraphDev {         // one resident problem
    uint64_t arena_off;      // first byte of its arena in the batch's arena buffer (a multiple of 8)
    uint64_t out_off;        // first byte of its consensus string among the batch's strings (capacity: bound)
    uint32_t seq_first;      // its first sequence's PoaSeqDev
    uint32_t n_seq;
    uint32_t bound;          // capacity in nodes and in edges (1..65535)
    uint32_t n_nodes, n_edges;
    uint32_t err;            // kPoaErr* bits; once set the kernels leave the problem alone and the host path computes it
};
struct PoaSeqDev {
    uint64_t off;            // first byte in the batch's sequence pool; a NUL follows the last byte
    uint32_t len, pad_;
};
struct PoaRoundDev {         // one problem of a round, in the order of the round's launches
    uint32_t prob, pad_;
    uint64_t cell_off;       // first cell of its (X + 1)(Y + 1) scores / origins in its launch
};
struct PoaXeDev {            // what the host reads per problem and round: 8 bytes
    uint32_t X;              // nodes of the graph (rows of the next alignment)
    uint32_t err;
};
enum : uint32_t {            // PoaGraphDev::err -- a capacity of the arena reached or a trip bound of a data-dependent loop
    kPoaErrNodes = 1u, kPoaErrEdges = 2u, kPoaErrList = 4u, kPoaErrStack = 8u, kPoaErrTrips = 16u, kPoaErrOrder = 32u, kPoaErrRoute = 64u,
    kPoaErrPreds = 128u
};
// start: the first sequence as a chain, the identity order (n problems).  rows: rank, rows, predecessor rows, sink flags and the
// PoaJobDev K13 reads (jobs[prob]) for sequence r of the round's problems.  thread: the route K13 left threaded through the graph,
// the new order.  consensus: heaviest path and string of problems ids[0 .. n), out_len[prob] = its length (cut at the first NUL).
void launch_poa_graph_start(PoaGraphDev *graphs, PoaXeDev *xe, unsigned char *arena, const char *seqs, const PoaSeqDev *seq_tab, int n,
                            void *stream);
void launch_poa_graph_rows(PoaGraphDev *graphs, const PoaRoundDev *round, int n_round, uint32_t r, unsigned char *arena,
                           const PoaSeqDev *seq_tab, PoaJobDev *jobs, void *stream);
void launch_poa_graph_thread(PoaGraphDev *graphs, PoaXeDev *xe, const PoaRoundDev *round, int n_round, uint32_t r, unsigned char *arena,
                             const char *seqs, const PoaSeqDev *seq_tab, const PoaJobDev *jobs, void *stream);
void launch_poa_graph_consensus(PoaGraphDev *graphs, const uint32_t *ids, int n, unsigned char *arena, char *out, uint32_t *out_len,
                                void *stream);

// ---- scoring DP (K10), segment-parallel: see the head comment of the K10 section in msa_kernels.hip ----
struct SegItem {            // work item of the segment kernel
    uint32_t pile;
    uint32_t seg;
};
struct SegSum {             // one per (pile, segment)
    // written by the kernel that scored the segment
    int32_t vmin, amax;           // smallest offset-carrying / largest absolute link score from the column before the segment on
    int32_t bmax_rel, bmax_abs;   // largest cell best of the segment by kind (INT32_MIN: none)
    uint32_t links;               // distinct links of the segment's columns
    uint32_t n_fin;               // links of its last column (entries of `fin`)
    uint32_t flags;               // 1: a column does not fit the LDS tables, 2: a raw score left the int32 working range
    // written by the stitch kernel
    int32_t dlt;                  // constant between the predecessor's `fin` and this segment's `spec`
    uint32_t ok;                  // the boundary check passed
    uint32_t enc;                 // 1: raw scores above kRelThr carry `off`
    long long off;                // true score = raw + off
};
struct K10Args {
    PileDev *piles;
    const uint32_t *coverage, *max_size, *cell_base, *ent_base, *cell_start, *cell_len, *ent_pp, *ent_ppp, *ent_cnt;
    uint32_t *cell_best_pp, *cell_best_link;
    int32_t *cell_best;           // best score of every cell (raw)
    SegSum *sums;
    int32_t *spec, *fin;          // kSegEnts raw scores per segment: what it held for the column before its first / computed for its last
    uint32_t seg_len, warm;       // columns per segment, warm-up columns of a speculative segment (< seg_len)
    int32_t guard;                // raw scores beyond it send the pile to the int64 kernel
    uint32_t force_repair;        // test hook: every segment with index % force_repair == 1 is treated as failed
};
constexpr int kSegEnts = 512;     // = the large tier's link slots per column

struct PathItem {           // one visited cell of the best_pp walk (origin first)
    uint32_t tag;           // packed (t_pos, delta, base)
    uint16_t link;          // best_link_count of the cell
    uint16_t cov;           // coverage of the column
};

// ---- K20: consensus words and low-quality windows of the walk (cns_windows_kernel, msa_kernels.hip; the rule: nd_cns.h) ----
struct CnsJobDev {          // one walk
    uint64_t path_off;      // its first PathItem, and its first word in the per-walk word slices (piles given: taken from PileDev)
    uint64_t win_off;       // its first window slot (two words a window: start, end)
    uint32_t n;             // items of the walk (piles given: the capacity of its slice; the length is PileDev::path_len)
    uint32_t win_cap;       // window slots: (capacity in items) / 24 + 1, see the kernel
    int32_t min_cov;
    uint32_t lq_max_len;
    uint32_t pile;          // piles given: the walk's PileDev
    uint32_t decline;       // test hook: the kernel leaves the walk with kCnsErrHook
};
struct CnsOutDev {          // what the host reads per walk: 32 bytes
    uint32_t len, uncorrected_len, lstrip, rstrip, lqseq_total_length;
    uint32_t n_win;
    uint32_t err;           // kCnsErr* bits; nonzero: declined, the host routine takes the walk
    uint32_t visited;       // items the window automaton stepped through (the rest it skipped from its idle state)
};
constexpr int kCnsLqMinLength = 8;   // lq_min_length (lib/nextcorrect.c:1890)
enum : uint32_t { kCnsErrWindows = 1u, kCnsErrTrips = 2u, kCnsErrCov = 4u, kCnsErrHook = 8u, kCnsErrLen = 16u };
// K20 over jobs [0, n): words[path_off + p] = pos << 8 | char, wins[2 (win_off + k)] = start, [.. + 1] = end, out[i].  piles != nullptr: job i reads
// path_off and n from piles[jobs[i].pile] (the walk where bt_emit left it).  Then the gather: job i's words to dense_words at the sum of
// the lengths in front of it, its windows to dense_wins at the sum of the window counts (declined walks count as empty).
void launch_cns_windows(const CnsJobDev *jobs, const PileDev *piles, const PathItem *path, uint32_t *words, uint32_t *wins, CnsOutDev *out,
                        uint32_t *dense_words, uint32_t *dense_wins, int n, void *stream);

// ---- K21: the HiFi and -fast forms of the loop behind the walk (cns_walk_kernel, msa_kernels.hip; the rules: nd_cns.h) ----
enum : uint32_t { kCnsModeRaw = 0u, kCnsModeHifi = 1u, kCnsModeFast = 2u };   // (raw is K20's: K21 declines it with kCnsErrMode)
struct CnsWalkJobDev {      // one walk: CnsJobDev's fields, the mode and where the seed's codes are
    uint64_t path_off;      // its first PathItem, its first word (HiFi) and its first character (-fast) in the per-walk slices
    uint64_t win_off;       // its first window slot
    uint64_t seed_off;      // piles not given, HiFi: the first of the seed's byte codes in `seed_codes`
    uint32_t n;             // items of the walk (piles given: the capacity of its slice)
    uint32_t win_cap;       // window slots: (capacity in items) / 6 + 1, see the kernel
    int32_t min_cov;
    uint32_t mode;          // kCnsMode*
    uint32_t pile;          // piles given: the walk's PileDev (HiFi: the seed's codes come from its packed bases)
    uint32_t decline;       // test hook
    uint32_t seed_len;      // piles not given, HiFi: codes at seed_off
    uint32_t pad_;
};
struct CnsWalkOutDev {      // what the host reads per walk: 32 bytes
    uint32_t len;           // HiFi: consensus bases; -fast: characters emitted (the walk is cut where the tenth slot would open)
    uint32_t lqseq_total_length;   // HiFi: bases with cov < 4, qv < 80 or another base than the seed's; -fast: lq_total_len of the result
    uint32_t n_win;         // HiFi: windows
    uint32_t err;           // kCnsErr* bits; nonzero: declined
    uint32_t lq_m, hq_m;    // -fast: the chosen stretch of the emitted string
    uint32_t n_words;       // words the gather writes for the walk (HiFi: len) ...
    uint32_t n_bytes;       // ... and bytes (-fast: hq_m - lq_m)
};
enum : uint32_t { kCnsErrSeed = 32u, kCnsErrMode = 64u, kCnsErrRange = 128u };   // (beside K20's bits)
// K21 over jobs [0, n), then its gather: words and windows as K20's, the -fast strings (each [lq_m, hq_m) reversed) to dense_seq at the
// sum of n_bytes in front.  piles != nullptr: path_off, the length and (HiFi) the seed's 2-bit codes in pool / db_pool come from
// piles[jobs[i].pile]; otherwise the HiFi seeds are byte codes in seed_codes.
void launch_cns_walk(const CnsWalkJobDev *jobs, const PileDev *piles, const PathItem *path, const uint32_t *pool, const uint32_t *db_pool,
                     const uint8_t *seed_codes, uint32_t *words, uint32_t *wins, uint8_t *chars, CnsWalkOutDev *out, uint32_t *dense_words,
                     uint32_t *dense_wins, uint8_t *dense_seq, int n, void *stream);

// ---- K24: the splice, its table of lower-case runs and the terminal SSR trim (splice_kernel, msa_kernels.hip; the rule: nd_splice.h) ----
struct SpliceRegDev {       // one region of a job, in the engine's order
    uint32_t start, end;    // inclusive positions
    uint32_t seed_off;      // its pseudo-seed's first byte behind the job's seed_off
    uint32_t seed_len;
    uint32_t usable;        // len > 0 or len == -2
    uint32_t reach;         // 1 + the largest end (capped at 2^21) among the usable regions of this index and above; 0: there is none
};
struct SpliceJobDev {
    uint64_t word_off;      // the first word the loop reads (the word at lstrip)
    uint64_t reg_off;       // its first SpliceRegDev
    uint64_t seed_off;      // its pseudo-seed bytes
    uint64_t out_off;       // its slice of the emitted characters
    uint32_t n_words;       // len - lstrip - rstrip
    uint32_t n_regions;
    uint32_t out_cap;       // n_words + the usable regions' pseudo-seed bytes: a region is emitted once at most
    uint32_t hifi;
    uint32_t decline;       // test hook: the kernel leaves the job with kSpliceErrHook
    uint32_t pad_;
};
struct SpliceOutDev {       // what the host reads per job: 48 bytes
    uint32_t err;           // kSpliceErr* bits; nonzero: declined, splice_host takes the job
    uint32_t out_len;       // characters emitted (cut where the tenth slot would open)
    uint32_t lq_m, hq_m;    // the chosen stretch
    uint32_t lq_total_len;
    int32_t lq_i;
    int32_t clip_s, clip_e;
    uint32_t code;          // 0, or the outcomes 2 (HiFi: all lower case) and 4 (the clips leave 10 bases or fewer)
    uint32_t trimmed;       // the gate let the trim run
    uint32_t n_bytes;       // bytes the gather writes for the job ...
    uint32_t src;           // ... from this index of its emitted characters on
};
enum : uint32_t { kSpliceErrHook = 1u, kSpliceErrCap = 2u, kSpliceErrRange = 4u };
// K24 over jobs [0, n), then its gather: job i's result string to dense_seq at the sum of n_bytes in front of it (declined jobs count as empty).
void launch_splice(const SpliceJobDev *jobs, const uint32_t *words, const SpliceRegDev *regs, const uint8_t *seeds, uint8_t *chars,
                   SpliceOutDev *out, uint8_t *dense_seq, int n, void *stream);

struct ColBlock {           // work item of the link-counting kernel
    uint32_t pile;
    uint32_t col0;
};

struct RegionDev {          // low-quality region whose candidate strings are wanted
    uint32_t pile;
    uint32_t start, end;    // inclusive seed columns
    uint32_t max_len;       // lqseq_max_length
    uint32_t max_len0;      // limit for the seed's own candidate (HiFi: DAG_MAX_LENGTH, else = max_len)
    // outputs
    uint32_t n_ok;          // candidates written (<= 40)
    uint32_t n_large;       // reads that exceeded max_len before the 40th candidate
    uint32_t cand_off[40];  // byte offsets into the string pool
    uint16_t cand_len[40];
    uint16_t cand_rank[40]; // position of the source read among the pile's aligned reads
    // K14 (lq_rank_kernel): in: want_rank; out: the 8-mer ranking of the candidates, where ranked != 0
    uint16_t rank_kscore[40];
    uint8_t rank_order[40];
    uint8_t want_rank, ranked, rank_tail, pad_;
};

constexpr int kColBlock = 32;          // columns per link-counting work item
// Distinct (pp, ppp) links per cell that the link-counting kernel holds in LDS: kLinkCapSmall in its first attempt, kLinkCap in
// its second.  Neither is a bound.  The reference has none (lib/nextcorrect.c:163-167 grows a cell's list by realloc, five links at
// a time).  What its rules do bound: an accepted read puts at most one tag into a cell, so a cell has at most as many links as
// its column has reads; the admission cut (total aligned length / seed length > max_cov_aln, :2271) bounds the AVERAGE depth, so
// windows of min_len_aln bases on one spot of a long seed stack max_cov_aln x seed_len / min_len_aln reads on a column; and a
// tag in front of a column is (column - 1, delta, base) with delta <= 250 (a longer gap fails the alignment, lib/align.c:542-545),
// about 1,000 values of pp alone.  Assembled read sets stay far below either capacity, because reads agree on what stands in
// front of a column.  A pile built for it does not: 192 reads on one window that each carry an insertion in front of the same
// column, 96 lengths closed by one of two bases, so that the link differs by (length, last base)
// (tests/golden/make_edge_piles_golden.py, family `links`: 201 records, default arguments, coverage 87), and the reference
// corrects it.  So a sub-batch whose cell overflows kLinkCap is counted a third time by count_links_global_kernel, whose lists
// live in device memory and hold one entry per accepted read of the deepest pile; the family `stack` runs it with more than 600.
constexpr int kLinkCap = 192;
constexpr int kLinkCapSmall = 64;
// Words of the link counter's error block: [0] a cell overflowed its lists; [1..4] what count_links_kernel's blocks did (blocks
// on the compact path, blocks on the deep path, largest cover among the former, ~(smallest cover among the latter), 0: none).
constexpr int kErrWords = 8;
constexpr int kLinkGlobalGrid = 1024;  // blocks of the third attempt (each owns 18 lists of `cap` words)

void launch_shift_scan(const AlnTask *tasks, const AlnOut *outs, const uint32_t *ops, ReadDev *reads, int n_reads,
                       void *stream);
void launch_pile_accept(PileDev *piles, ReadDev *reads, uint32_t *acc_list, uint32_t *cov_diff, int n_piles,
                        void *stream);
void launch_make_tags(const PileDev *piles, const ReadDev *reads, const AlnTask *tasks, const uint32_t *ops,
                      const uint32_t *pool, const uint32_t *db_pool, const uint32_t *read_pile, uint32_t *tags,
                      uint32_t *colidx, uint32_t *ins_count, uint32_t *ins_max, int n_reads, void *stream);
// in: cov_diff (difference array), ins_max; out (in place): coverage, max_size; plus offsets
void launch_col_scan(PileDev *piles, uint32_t *cov_diff, const uint32_t *ins_count, uint32_t *ins_max,
                     uint32_t *cell_base, uint32_t *ent_base, int n_piles, void *stream);
// What the link counter (K9) reads and the five tables it writes: one record for its two launches, the digest hook and the fields
// K10Args shares with them (k10_args_from).  The kernels keep their flat parameter lists; the wrappers unpack the record.
struct K9Args {
    PileDev *piles;
    const ReadDev *reads;
    const uint32_t *acc;          // accepted reads of every pile
    const ColBlock *blocks;
    const uint32_t *tags, *colidx, *max_size, *cell_base, *ent_base;
    uint32_t *cell_start, *cell_len, *ent_pp, *ent_ppp, *ent_cnt;   // the tables
    uint32_t *err;                // kErrWords words, zero before the launch
};
inline K10Args k10_args_from(const K9Args &k) {   // (coverage, the cell bests, the segment buffers and the knobs are the caller's)
    K10Args a{};
    a.piles = k.piles, a.max_size = k.max_size, a.cell_base = k.cell_base, a.ent_base = k.ent_base;
    a.cell_start = k.cell_start, a.cell_len = k.cell_len, a.ent_pp = k.ent_pp, a.ent_ppp = k.ent_ppp, a.ent_cnt = k.ent_cnt;
    return a;
}
// A column block that at most NDGPU_K9_COMPACT (0..64, default 64; read once) accepted reads reach is counted on the compact path
// -- one lane per covering read --, any other by the loop over all accepted reads.
void launch_count_links(const K9Args &a, int n_blocks, bool full_capacity, void *stream);
void launch_count_links_global(const K9Args &a, uint32_t *lists, uint32_t cap, int n_blocks, int grid, void *stream);
// Trace hook (NDGPU_K9_DIGEST): what the link counter left in its tables, for piles [0, n_piles).  out[0] += a hash of every cell's
// (pile, cell, start, len) and of every (pile, cell, position, pp, ppp, cnt) of its links [start, start + len) -- position-dependent,
// summed, so the same whatever the order of the blocks; out[1] += cells, out[2] += links, out[3] = max(len).  out: zero before.
void launch_k9_digest(const K9Args &a, unsigned long long *out, int n_piles, void *stream);
// segment kernels of both table tiers (the large one on stream_large at the same time) -> stitch -> int64 kernel for
// the piles they left (err == 2) -> best_pp walk
// (ent_score == nullptr: the int64 kernel is not launched and leaves err == 2 piles for a second call with rescue = true,
// which launches only that kernel and the walk) then the best_pp walk, cut at the same segments: items_all = every (pile, segment) of the launch, bt_exit / bt_steps =
// kBtSlots entries per segment, bt_entry / bt_off = one per segment
void launch_score_backtrack(const K10Args &a, const SegItem *items_small, int n_small, const SegItem *items_large, int n_large,
                            const SegItem *items_all, int n_all, long long *ent_score, bool rescue, PathItem *path, uint32_t *bt_exit,
                            uint32_t *bt_steps, uint32_t *bt_entry, uint32_t *bt_off, int n_piles, void *stream,
                            void *ev_after_fast, void *stream_large, void *ev_fork, void *ev_join);
constexpr int kBtSlots = 192;
void launch_extract(const PileDev *piles, const ReadDev *reads, const uint32_t *acc_list, const uint32_t *tags,
                    const uint32_t *colidx, RegionDev *regions, char *strpool, unsigned long long *strpool_cursor,
                    unsigned long long strpool_cap, int n_regions, void *stream);

// K14: ranks the candidates of every region with want_rank and min_n <= n_ok <= 40 whose strings lie inside strpool[0, strpool_cap)
void launch_lq_rank(RegionDev *regions, const char *strpool, unsigned long long strpool_cap, uint32_t min_n, int n_regions, void *stream);

// ---- K22: the phasing and ranking of a HiFi pile's candidates (hifi_phase_kernel + hifi_phase_rank_kernel, lq_kernels.hip; the
// rule: hifi_phase_host of nd_phase.h) ----
// A pile's table of per-read phase scores lives in LDS, two words a read: a pile with more aligned reads is declined.
constexpr uint32_t kPhaseReads = 2048;
constexpr uint32_t kPhaseRegionsMax = 65535;   // beyond: the reference's 16-bit scores may wrap; declined
typedef PhaseRecord PhaseRegionDev;            // one per region, indexed like the launch's RegionDev records
struct PhasePileDev {       // one pile that asks: 32 bytes
    uint32_t first_region;  // its regions are RegionDev / PhaseRegionDev [first_region, first_region + n_regions)
    uint32_t n_regions;
    uint32_t n_aligned;
    uint32_t decline;       // test hook: the kernel leaves the pile with kPhaseErrHook
    // outputs
    uint32_t err;           // kPhaseErr* bits; nonzero: declined, the host rule takes the pile
    uint32_t has_heter, pass2;
    uint32_t pad_;
};
enum : uint32_t {
    kPhaseErrReads = 1u,    // n_aligned > kPhaseReads
    kPhaseErrRegions = 2u,  // n_regions > kPhaseRegionsMax
    kPhaseErrPool = 4u,     // a candidate's bytes lie outside the string pool, or a region has more than 40 candidates
    kPhaseErrHook = 8u,
    kPhaseErrSource = 16u   // a candidate's source read is not below n_aligned
};
constexpr uint32_t kPhaseWorkWords = 40;       // words of work state per region between the kernel's steps
constexpr uint8_t kPhasePending = 255;         // (device only) PhaseRecord::kind of a region that waits for its ranking
// work: kPhaseWorkWords words per region; out is cleared by the caller before the launch
void launch_hifi_phase(const RegionDev *regions, const char *strpool, unsigned long long strpool_cap, PhasePileDev *piles, int n_piles,
                       PhaseRegionDev *out, uint32_t *work, int n_regions, void *stream);

constexpr uint64_t kOffDb = 1ull << 63;   // offset flag: sequence lives in the resident read DB
constexpr uint64_t kOffMask = kOffDb - 1;

// Words of zeros behind the last sequence of every 2-bit pool (per-batch pools, the resident read DB): the forward kernel fetches 64
// bases -- five words -- at a time, starting anywhere up to the last base (csrc/ond_kernels.hip: fetch64_rel), and a walker of the
// traceback fills its window with the 16 words from a sequence's first on, however short the sequence (fetch64_win)
constexpr uint32_t kPoolPadWords = 24;
constexpr uint32_t kTracePadWords = 16;  // words behind the last task's trace: a walker's window holds 16 record words from the task's first on
constexpr int kFastRowWords = 2;       // register path: at most two 64-bit trace words per edit step (one up to 56 cells)
constexpr int kFastMaxBand = 238;      // register path: at most 120 same-parity diagonals per edit step (two per lane, 7-bit offsets)

// launchers (ond_kernels.hip)
void launch_ond_forward(const AlnTask *tasks, AlnOut *outs, const uint32_t *pool, const uint32_t *db_pool,
                        uint64_t *trace, int n_tasks, void *stream, const int32_t *order = nullptr);  // order: device, n_tasks ids, longest first
// The forward kernel with checkpoints + the traceback in segments (chase, walkers, stitch, and the one-lane walk for what the stitch
// refuses).  ck_cells: kCkptCells words per checkpoint slot, ck_hdr: one uint2 per slot (AlnTask::mink_off = a task's first slot,
// ((max_d - 1) >> cshift) slots each); segs / seg_outs: AlnTask::seg_off = a task's first walker slot, slots + 1 each; n_slots = all of them.
struct TbArgs {
    uint32_t *ck_cells;
    void *ck_hdr;
    TbSeg *segs;
    TbSegOut *seg_outs;
    int n_slots;
    int cshift, warm;
};
void launch_ond_forward_ckpt(const AlnTask *tasks, AlnOut *outs, const uint32_t *pool, const uint32_t *db_pool, uint64_t *trace,
                             uint32_t *ops, const TbArgs &tb, int n_tasks, void *stream, const int32_t *order);
void launch_ond_traceback_seg(const AlnTask *tasks, AlnOut *outs, const uint32_t *pool, const uint32_t *db_pool, const uint64_t *trace,
                              uint32_t *ops, const TbArgs &tb, int n_tasks, void *stream);
void launch_ond_forward_wide(const AlnTask *tasks, AlnOut *outs, const uint32_t *pool, const uint32_t *db_pool,
                             uint64_t *trace, int32_t *trace_mink, int32_t *vscratch, const int32_t *task_ids, int n_ids, void *stream,
                             const AlnTask *wtasks = nullptr, uint32_t max_ring = 0);
constexpr size_t kWideLdsBytes = 64u << 10;   // the wide path keeps V rings up to this size in LDS (a workgroup's default limit)  // wtasks: the listed tasks' records (wide-path fields), in list order
// task_ids == nullptr: tasks [0, n), traces in the register path's stream format, walked in the order `order` lists them
// (device, n ids; nullptr = table order); otherwise the listed (wide-band) tasks, traces in the wide kernel's row format
void launch_ond_traceback(const AlnTask *tasks, AlnOut *outs, const uint32_t *pool, const uint32_t *db_pool,
                          const uint64_t *trace,
                          const int32_t *trace_mink, uint32_t *ops, const int32_t *task_ids, int n, void *stream,
                          const int32_t *order = nullptr, const AlnTask *wtasks = nullptr);

// ---- K15: the traceback's column stream as runs (aln_runs_kernel, ond_kernels.hip) ----
// What a batch caller takes home instead of one byte per column: per task the counts of its columns by kind, its runs of equal kinds
// and the longest gap run, and the runs themselves as BAM-numbered uint32 (length << 4 | op).
struct AlnRunSum {
    uint32_t n_runs;        // runs of equal column kinds (ST_ALIGNED: all n_cols columns; ST_GAP_ABORT: the last two; otherwise 0)
    uint32_t n_match, n_ins, n_del;   // columns of OP_MATCH / OP_QONLY / OP_TONLY among them
    uint32_t max_gap_run;   // the longest run of OP_QONLY or of OP_TONLY columns
    uint32_t aln_len;       // the columns counted
};
constexpr uint32_t kCigarEq = 7, kCigarIns = 1, kCigarDel = 2;   // '=' for OP_MATCH (a diagonal step of O(ND) is an equal pair), 'I', 'D'
// count pass: sums[i] of every task i of [0, n_tasks); skip (may be nullptr): bit i set = task i counts as not aligned
void launch_aln_runs_count(const AlnTask *tasks, const AlnOut *outs, const uint32_t *ops, const uint32_t *skip, AlnRunSum *sums, int n_tasks,
                           void *stream);
// emit pass: task i writes its sums[i].n_runs runs to runs[run_off[i] ...] (run_off: the exclusive scan of n_runs)
void launch_aln_runs_emit(const AlnTask *tasks, const AlnOut *outs, const uint32_t *ops, const AlnRunSum *sums, const uint64_t *run_off,
                          uint32_t *runs, int n_tasks, void *stream);

}  // namespace ndgpu
