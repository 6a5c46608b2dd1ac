/* ndgpu_nextcorrect.h -- C ABI of the MI355X-native read-correction engine.
 *
 * Drop-in boundary: the symbols below are exactly what NextDenovo's correction
 * stage binds through ctypes (reference lib/nextcorrect.py:56-59) and what
 * minimap2-nd / ctg_cns link against (reference lib/align.h:45-62).  Build
 * product: nextdenovo_amd/libndgpu_nextcorrect.so (install it as lib/nextcorrect.so
 * next to lib/nextcorrect.py).
 *
 * All compute behind these entry points runs in hand-written HIP kernels on
 * gfx950; there is no CPU fallback: the first call aborts with a message if no
 * HIP device is visible.
 */
#ifndef NDGPU_NEXTCORRECT_H
#define NDGPU_NEXTCORRECT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these are its only exports */

/* replaces: reference lib/nextcorrect.h:70-74 (`consensus_trimed`), mirrored by
 * lib/nextcorrect.py:19-24.  `seq` is malloc'd, NUL-terminated, mixed case
 * (lower case = low confidence).  len 2 = uncorrectable, 3 = out of memory,
 * 4 = everything clipped (lib/nextcorrect.c:2254-2261, 1999, 2126). */
typedef struct {
    unsigned int len;
    float identity;
    char *seq;
} consensus_trimed;

/* replaces: reference lib/nextcorrect.h:161-162 / lib/nextcorrect.c:2219-2305.
 * seqs[0] = full seed, seqs[i>0] = strand-corrected overlapping substrings (ASCII,
 * upper-case ACGT, NUL-terminated); aln_start/aln_end = inclusive seed coordinates.
 * read_type: 1 ont, 2 clr, 3 hifi. */
consensus_trimed *nextCorrect(char **seqs, unsigned int *aln_start, unsigned int *aln_end, unsigned int seq_count,
                              unsigned int max_mem_len, unsigned int min_len_aln, unsigned int max_cov_aln,
                              unsigned int min_cov, unsigned int lqseq_max_length, float min_error_corrected_ratio,
                              unsigned int split, unsigned int fast, int read_type);

/* replaces: reference lib/nextcorrect.h:164 / lib/nextcorrect.c:2307-2310 */
void free_consensus_trimed(consensus_trimed *c);

/* ---- lib/align.h family (short `alignment` layout, i.e. without -DLGS_CORRECT,
 *      reference lib/align.h:21-32 / lib/nextcorrect.h:120-129) ---- */
typedef struct {
    unsigned int shift;
    unsigned int aln_len;
    unsigned int aln_t_s;
    unsigned int aln_t_e;
    unsigned int aln_t_len;
    unsigned int aln_q_len;
    char *q_aln_str;
    char *t_aln_str;
} alignment;

/* replaces: reference lib/align.h:61-62 / lib/align.c:572-578.  V and D are accepted
 * for signature compatibility and ignored (the device keeps its own state). */
void align(char *query_seq, int q_len, char *target_seq, int t_len, alignment *align_rtn, int *V, uint8_t **D);
/* replaces: reference lib/align.h:59-60 / lib/align.c:563-570 */
void align_hq(char *query_seq, int q_len, char *target_seq, int t_len, alignment *align_rtn, int *V, uint8_t **D);
/* replaces: reference lib/nextcorrect.h:157 / lib/align.c:580-679: full-matrix global alignment (match 2, mismatch -4, gap
 * open -4, gap extend -2).  s1 indexes the columns and is written to q_aln_str, s2 to t_aln_str; only aln_len and the two
 * strings (caller-allocated, s1_l + s2_l + 1 bytes each) are set.  Host routine: the reference calls it from nowhere. */
void align_nd(const char *s1, const uint32_t s1_l, const char *s2, const uint32_t s2_l, alignment *aln);
/* replaces: reference lib/align.h:45-50 / lib/align.c:22-78 (host-only helpers) */
void malloc_vd(int **V, uint8_t ***D, uint64_t max_mem_d);
void clean_V(int *V, int max_mem_d);
void destory_vd(int *V, uint8_t **D);
void revcomp_bseq(char *str, int len);
void reverse_str(char *str, int len);
void str_tolower(char *p);
void str_toupper(char *p);
/* ---- the prefix / extension members of the O(ND) family (reference lib/align.h:36-58, lib/align.c:80-426; callers
 *      minimap2/map.c:385-482, 941-956 and lib/ctg_cns.c).  GPU-backed (csrc/ext_kernels.hip); V and D are ignored. ---- */
typedef struct {
    unsigned int aln_len;  /* alignment columns */
    unsigned int aln_mlen; /* matching columns */
    unsigned int aln_t_s;
    unsigned int aln_t_e;  /* exclusive */
    unsigned int aln_q_s;
    unsigned int aln_q_e;  /* exclusive */
} alignpos;
/* replaces lib/align.c:80-141: *mlen / *blen are written when either sequence is exhausted within max_d steps and the band cap */
void ide(const char *query_seq, int q_len, const char *target_seq, int t_len, int *V, uint8_t **D, int max_d, int band_size,
         int *mlen, int *blen);
/* replaces lib/align.c:146-253: *aln is written under the same condition */
void alnpos(const char *query_seq, int q_len, const char *target_seq, int t_len, int *V, uint8_t **D, int max_d, int band_size,
            alignpos *aln);
/* replace lib/align.c:256-340 / :343-426: (*bstx, *bsty) = query / target bases covered at the peak of (x + y) * d_factor - d */
void extend_fwd(const char *query_seq, int q_len, const char *target_seq, int t_len, int *V, uint8_t **D, int max_d, int band_size,
                float d_factor, int *bstx, int *bsty);
void extend_rev(const char *query_seq, int q_len, const char *target_seq, int t_len, int *V, uint8_t **D, int max_d, int band_size,
                float d_factor, int *bstx, int *bsty);
/* additive: a batch of such problems in one launch (one lane per problem) -- what nd_extend_ends' loop over the overlaps of a read
 * (minimap2/map.c:385-482) would hand over.  kind: 0 ide, 1 alnpos, 2 extend_fwd, 3 extend_rev.  result: done = an end condition
 * fired; (a, b) = (mlen, blen) or (bstx, bsty); pos[6] = the fields of `alignpos` (alnpos only).  Returns 0, < 0 on error. */
typedef struct ndgpu_ext_job {
    const char *q;
    int32_t q_len;
    const char *t;
    int32_t t_len;
    int32_t max_d, band_size;
    float d_factor;
    int32_t kind;
} ndgpu_ext_job;
typedef struct ndgpu_ext_result {
    int32_t done, a, b;
    uint32_t pos[6];
} ndgpu_ext_result;
int ndgpu_ext_batch(const ndgpu_ext_job *jobs, int n, ndgpu_ext_result *res);

/* replaces: reference lib/nextcorrect.h:166 / lib/dag.c:658-694.  `seqs` points at
 * `seq_count` records laid out as the reference's `struct seq_`
 * (lib/nextcorrect.h:63-68: u16 order, u16 kscore, u16 len, char seq[10000]).
 * A host routine: one small problem is not worth a kernel launch.  Many problems at once: ndgpu_poa_batch below. */
char *poa_to_consensus(const void *seqs, const int seq_count);

/* ---- additive entry points (not in the reference) ---- */

/* Correct `n_piles` seeds in one call so that thousands of alignments share each
 * kernel launch.  Per-pile arguments are arrays of length n_piles whose elements have
 * the meaning of the corresponding nextCorrect() argument; scalar options apply to all
 * piles.  out[i] receives a malloc'd consensus_trimed (free with
 * free_consensus_trimed).  host_threads <= 0 selects hardware concurrency.
 * Returns 0. */
int ndgpu_correct_batch(int n_piles, char ***seqs, unsigned int **aln_start, unsigned int **aln_end,
                        const unsigned int *seq_count, const unsigned int *max_mem_len,
                        const unsigned int *lqseq_max_length, unsigned int min_len_aln, unsigned int max_cov_aln,
                        unsigned int min_cov, float min_error_corrected_ratio, unsigned int split, unsigned int fast,
                        int read_type, int host_threads, consensus_trimed **out);

/* poa_to_consensus for many problems in one call: the alignment of every further sequence against its problem's graph -- the
 * O(X * Y) step -- runs on the device, sequence r of all problems in one launch; graph growth, topological order and heaviest path stay
 * on the host.  Sequences are len[k] bytes each (1..9,999 on the device; a problem with another length, or too large for the device
 * memory plan, is computed by the host routine inside the same call), at most 64 per problem.
 * out[i]: malloc'd, NUL-terminated, what poa_to_consensus returns for job i's sequences.  Returns 0, < 0 on error. */
typedef struct ndgpu_poa_job { const char *const *seqs; const uint16_t *len; int32_t seq_count; } ndgpu_poa_job;
int ndgpu_poa_batch(const ndgpu_poa_job *jobs, int n, char **out);
/* The same call with a choice of path; ndgpu_poa_batch is this call with flags 0.
 *   bit 0: the host routine for every job, no device work (the cross-check leg);
 *   bit 1: resident graphs -- a problem's graph lives on the device from its first sequence to its consensus string: graph growth,
 *          topological order, the rows and the heaviest path run in kernels around the alignment, per round only 16 bytes a problem
 *          go up and 8 come down.  A problem whose node bound sum(len + 1) exceeds 65,535, or that does not fit the memory plan, takes
 *          the rounds of bit 2 inside the same call; one that reaches a capacity of its arena is computed by the host routine;
 *   bit 2: the rounds of ndgpu_poa_batch's first description: alignments on the device, graphs on the host.
 * Neither bit 1 nor bit 2: the environment variable NDGPU_POA_RESIDENT=1 (read once per process) selects bit 1's path, otherwise
 * bit 2's.  The bytes returned are the same on every path.  Bits 1 and 2 together, or any other bit: -2, nothing written. */
int ndgpu_poa_batch_flags(const ndgpu_poa_job *jobs, int n, int flags, char **out);

/* The 8-mer ranking of a low-quality region's candidates (reference lib/nextcorrect.c:281-337, 405-440) for many candidate sets in
 * one call, one wavefront per set on the device.  A job is seq_count (1..40) sequences of len[k] bytes (0..9,999) in input order;
 * only the first and last 40 bytes of a sequence are read.  res[i].order[r]: the input index of the sequence at rank r,
 * res[i].kscore[r]: its score (entries from seq_count on are 0), res[i].tail: whether the tail windows were ranked too.
 * flags bit 0: compute with the engine's own host routine instead of the device.
 * Returns 0; < 0, with nothing written, when a job has seq_count outside 1..40 or no device can be used.  n = 0 is valid. */
typedef struct ndgpu_rank_job { const char *const *seqs; const uint16_t *len; int32_t seq_count; } ndgpu_rank_job;
typedef struct ndgpu_rank_result { uint8_t order[40]; uint16_t kscore[40]; int32_t tail; } ndgpu_rank_result;
int ndgpu_lq_rank_batch(const ndgpu_rank_job *jobs, int n, int flags, ndgpu_rank_result *res);

/* The consensus bases and low-quality windows of a main walk (the loop of generate_cns_from_best_score, reference
 * lib/nextcorrect.c:1907-1982: raw reads, not -fast) for many walks in one call, one wavefront per walk on the device.  A job is n steps
 * of a best_pp walk, origin first: seed position, best_link_count and coverage of the visited cell and its base code (A0 T1 G2 C3,
 * 4 a gap, 5 N).  res[i]: the five counters of the loop, n_regions windows from (*regions)[2 * region_off] on as (start, end) pairs of
 * seed positions in emission order, len words from (*bases)[base_off] on: pos << 8 | character (lower case: low coverage or quality),
 * numbered as the reference numbers them before reverse_consensus_base; ok: the verdict of lib/nextcorrect.c:1986-1987 with the job's
 * min_error_corrected_ratio.  *bases and *regions are one malloc'd block each, of exact size (free() them; one word when empty).
 * flags bit 0: the engine's own host routine instead of the device (the same result; a cross-check).
 * Returns 0; -2, with nothing computed or written, when n < 0, a pointer is NULL with n > 0, or a non-gap step has cov 0, a base above 5
 * or a t_pos outside 0 .. 2^21 - 2; < 0 when no device can be used.  n = 0 is valid. */
typedef struct ndgpu_walk_step { int32_t t_pos; uint16_t link, cov; uint8_t base; uint8_t pad_[3]; } ndgpu_walk_step;
typedef struct ndgpu_cns_job {
    const ndgpu_walk_step *steps;
    uint32_t n;
    int32_t min_cov;
    uint32_t lq_max_len;
    float min_error_corrected_ratio;
} ndgpu_cns_job;
typedef struct ndgpu_cns_result {
    uint32_t len, uncorrected_len, lstrip, rstrip, lqseq_total_length;
    int32_t ok;
    uint32_t n_regions, pad_;
    uint64_t base_off, region_off;
} ndgpu_cns_result;
int ndgpu_cns_windows_batch(const ndgpu_cns_job *jobs, int n, int flags, ndgpu_cns_result *res, uint32_t **bases, uint32_t **regions);

/* The loop behind a main walk in each of its three forms, for many walks in one call.  mode 0: raw reads -- exactly what
 * ndgpu_cns_windows_batch answers for the job's first five fields.  mode 1: HiFi reads (generate_cns_from_best_score_kmer, reference
 * lib/nextcorrect.c:1807-1860): the counters len and lqseq_total_length (the other three stay 0), words and windows as above (a window
 * may have been widened by a merge), ok: the verdict of :1864-1865; `seed` is the seed's ASCII bases, seed_len of them, read at every
 * non-gap step's t_pos through the engine's table (ACGT in either case 0..3 in the walk's numbering, N 5, M 6, anything else 4).
 * mode 2: -fast (generate_cns_from_best_score_fast, :1724-1777): len and identity as the engine reports them, lq_total_len, and len'
 * bytes from (*seqs)[seq_off] on, len' = seq_len: the chosen stretch of the emitted string, reversed; ok = 1; lq_max_len,
 * min_error_corrected_ratio and the seed are not read.  *bases, *regions as above; *seqs is one malloc'd byte block of exact size (free()
 * it; one byte when empty), the strings one behind the other without padding.  flags bit 0: the engine's host routines.
 * Returns 0; -2, with nothing computed or written, in the cases of ndgpu_cns_windows_batch, for a mode above 2, for mode 1 with a NULL
 * seed, and for mode 1 with a non-gap step whose t_pos >= seed_len; < 0 when no device can be used.  n = 0 is valid. */
typedef struct ndgpu_cns_walk_job {
    const ndgpu_walk_step *steps;
    uint32_t n;
    int32_t min_cov;
    uint32_t lq_max_len;
    float min_error_corrected_ratio;
    int32_t mode;
    uint32_t seed_len;
    const char *seed;
} ndgpu_cns_walk_job;
typedef struct ndgpu_cns_walk_result {
    uint32_t len, uncorrected_len, lstrip, rstrip, lqseq_total_length;
    int32_t ok;
    uint32_t n_regions, pad_;
    uint64_t base_off, region_off;
    uint32_t lq_total_len, seq_len;   /* mode 2 */
    float identity;
    uint32_t pad2_;
    uint64_t seq_off;
} ndgpu_cns_walk_result;
int ndgpu_cns_walk_batch(const ndgpu_cns_walk_job *jobs, int n, int flags, ndgpu_cns_walk_result *res, uint32_t **bases, uint32_t **regions,
                         char **seqs);

/* The end of a pile for many piles in one call: the splice of the regions' pseudo-seeds into the consensus with its table of
 * lower-case runs (update_consensus_trimed and update_lqreg, reference lib/nextcorrect.c:1340-1482) and the clipping of terminal
 * simple-sequence repeats (trim_terminal_ssr, :2008-2128).  A job holds the consensus words pos << 8 | char in ascending positions
 * (n_words of them; the loop reads [lstrip, n_words - rstrip)), its regions in the engine's order (the index counts down while the
 * positions go up; a region is usable when len > 0 or len == -2; sudoseed holds sudoseed_len bytes) and read_type (3: HiFi).
 * The result: len as the engine reports it (2: a HiFi string of lower case alone; 4: the clips leave 10 bases or fewer), lq_total_len
 * and identity as they stand before the trim, out_len (characters emitted before the stretch was chosen), the stretch [lq_m, hq_m),
 * lq_i, the two clips, and seq_len bytes from (*seqs)[seq_off] on: the result string (len 2: none; the len = 4 outcome of the trim:
 * the first four bytes of the untrimmed stretch, which is what the engine's record carries).  *seqs is one malloc'd byte block of
 * exact size (free() it; one byte when empty), the strings one behind the other.  flags bit 0: the host statement (nd_splice.h).
 * Returns 0; -2, with nothing computed or written, for n < 0, a NULL pointer with n > 0 (jobs, res, seqs, a job's words with
 * n_words > 0, its regions with n_regions > 0, a pseudo-seed with sudoseed_len > 0), lstrip + rstrip > n_words, descending positions
 * among the words read, and a region with start > end; < 0 when no device can be used.  n = 0 is valid.  A job the kernel must not
 * compute (a position above 2^21 - 2, more than 2^30 words and pseudo-seed bytes) is answered by the host statement. */
typedef struct ndgpu_splice_region {
    uint32_t start, end;
    int32_t len;
    uint32_t sudoseed_len;
    const char *sudoseed;
} ndgpu_splice_region;
typedef struct ndgpu_splice_job {
    const uint32_t *words;
    uint32_t n_words, lstrip, rstrip, n_regions;
    const ndgpu_splice_region *regions;
    int32_t read_type;
    uint32_t pad_;
} ndgpu_splice_job;
typedef struct ndgpu_splice_result {
    uint32_t len, lq_total_len;
    float identity;
    uint32_t out_len, lq_m, hq_m;
    int32_t lq_i, clip_s, clip_e;
    uint32_t seq_len;
    uint64_t seq_off;
} ndgpu_splice_result;
int ndgpu_splice_batch(const ndgpu_splice_job *jobs, int n, int flags, ndgpu_splice_result *res, char **seqs);

/* The phasing and ranking of the low-quality-region candidates of HiFi piles (generate_lqseqs_from_tags_kmer, lib/nextcorrect.c:787-948
 * with the helpers of 512-737: from the candidates as extracted up to the sort by score), for many piles in one call.  A job is a
 * pile: n_aligned reads, n_regions regions in order, each with its inclusive seed columns start / end and n_cand candidates (0..40):
 * bytes, lengths and source reads (each below n_aligned).  regions_out receives one record per region, the jobs' regions one behind
 * the other; piles_out one per job.  A record's kind is 0 (the region had no candidates), 1 (dropped: lq.len = 0), 2 (a candidate
 * becomes the pseudo-seed: seed is its input index, seed_pos its position, lower says that the pseudo-seed goes to lower case, n is
 * -2) or 3 (ranked: the first n positions reach the selection loop; tail says that the tail windows were ranked too).  perm[j] is the
 * input index of the candidate at position j of lq.seqs as the routine leaves it, kscore[j] its score as left by the last step that
 * wrote it, for every j below n_cand; indexs is the region's flag as the phasing left it.
 * flags bit 0: the engine's host rule; otherwise the device computes, and a pile it declines (more than 2,048 aligned reads, more
 * than 65,535 regions, or a pile of its own too large for the device's memory) takes the host rule.  Returns 0; -2, with nothing computed or written, for a NULL array, n_cand outside
 * 0..40, a NULL candidate of nonzero length, a source read not below n_aligned; < 0 when no device can be used.  n = 0 is valid. */
typedef struct ndgpu_phase_region_in {
    uint32_t start, end;
    int32_t n_cand;
    uint32_t pad_;
    const char *const *seqs;
    const uint16_t *len;
    const uint16_t *src;
} ndgpu_phase_region_in;
typedef struct ndgpu_phase_job {
    uint32_t n_aligned;
    uint32_t n_regions;
    const ndgpu_phase_region_in *regions;
} ndgpu_phase_job;
typedef struct ndgpu_phase_region {   /* 128 bytes */
    uint8_t kind, lower, indexs, tail;
    int16_t n;
    uint8_t seed, seed_pos;
    uint8_t perm[40];
    uint16_t kscore[40];
} ndgpu_phase_region;
typedef struct ndgpu_phase_pile {
    uint8_t has_heter;   /* a heterozygous site, or a candidate for one, was seen */
    uint8_t pass2;       /* ... and no SNP phased the seed: the second pass ran */
    uint8_t declined;    /* the device left the pile to the host rule */
    uint8_t pad_;
} ndgpu_phase_pile;
int ndgpu_hifi_phase_batch(const ndgpu_phase_job *jobs, int n, int flags, ndgpu_phase_region *regions_out, ndgpu_phase_pile *piles_out);

/* align() / align_hq() for many pairs in one call.  The pairs share the launches of the forward and traceback kernels; a further kernel
 * pair run-length-encodes every alignment's columns on the device, so that what comes back per job is its summary and its CIGAR, not a
 * byte per column.  res[i]: status (0: none -- align() would leave its argument untouched, which includes a sequence with a byte
 * outside ACGT; 1: aligned; 2: the > 250-gap abort, reported as align() reports it: aln_len 2, the last two columns), aln_len,
 * q_used / t_used (align()'s aln_q_len / aln_t_len), the columns by kind (n_match: equal pairs -- the O(ND) aligner has no mismatch
 * column; n_ins: query-only; n_del: target-only), max_gap_run (the longest run of one gap kind) and n_cigar runs from
 * (*cigar)[cigar_off] on: length << 4 | op in BAM numbering, 7 '=', 1 'I', 2 'D'.  *cigar is one malloc'd block (free() it).
 * hq != 0: align_hq's limits.  flags bit 0: the summaries and runs are computed on the host from the downloaded columns (the same
 * result; a cross-check).  flags bit 1: *q_aln / *t_aln receive one malloc'd block each with every job's gapped strings exactly as
 * align() writes q_aln_str / t_aln_str: job i's string starts at the sum of (aln_len + 1) over the jobs before it, is aln_len
 * bytes long and NUL-terminated (a job with status 0 has the NUL alone); without bit 1 q_aln / t_aln may be NULL.
 * Lengths are >= 0 and q_len + t_len < 2^28.  Returns 0; < 0, with nothing written, when n < 0, a pointer is NULL with n > 0, a length
 * is out of range, a DB job names a read or a window outside the DB, or no device can be used.  n = 0 is valid.
 * ndgpu_align_db_batch: both sides are windows of a resident read DB (inclusive ends, reverse-complemented when *_rev, as the
 * records of ndgpu_correct_piles name them): nothing is packed or uploaded. */
typedef struct ndgpu_aln_job { const char *q; int32_t q_len; const char *t; int32_t t_len; int32_t hq; } ndgpu_aln_job;
typedef struct ndgpu_aln_dbjob { uint32_t q_read, q_start, q_end, q_rev, t_read, t_start, t_end, t_rev; int32_t hq; } ndgpu_aln_dbjob;
typedef struct ndgpu_aln_result {
    int32_t status;
    uint32_t aln_len, q_used, t_used, n_match, n_ins, n_del, max_gap_run, n_cigar;
    uint64_t cigar_off;
} ndgpu_aln_result;
int ndgpu_align_batch(const ndgpu_aln_job *jobs, int n, int flags, ndgpu_aln_result *res, uint32_t **cigar, char **q_aln, char **t_aln);

/* The output loop of lib/nextcorrect.py:236-260 (without -s) over finished records: for every ids[k] in order, a record with
 * len >= min_len_seed, len > 4 and identity >= min_ratio is written to fd_out as ">NAME LEN IDENTITY\nBASES\n" (IDENTITY as Python's
 * '%f') and, if fd_idx >= 0, "NAME\tOFFSET\tLEN\n" to fd_idx (OFFSET = where the bases start in the output file); any other record
 * but an out-of-memory seed (len 3) gets "NAME\t0\t0\n" in the index.  names[i] = the number the reference prints for pile i;
 * *pos = the output file's size before the call, updated.  lens / identities (may be NULL) receive every handed-over record's
 * values at [ids[k]]; the records are freed (free_consensus_trimed) and their slots set to NULL.  What a caller's completion
 * callback (ndgpu_piles_done_fn) does with its sub-batch.  Returns 0, or -1 when a write fails. */
int ndgpu_write_records(consensus_trimed **recs, const uint32_t *ids, int n, const uint32_t *names, uint32_t min_len_seed,
                        double min_ratio, int fd_out, int fd_idx, uint64_t *pos, uint32_t *lens, float *identities);

/* Resident read database: the additive replacement for ovlseq.so's init_ovls + getseq
 * (reference lib/ovlseq.c:39-138, lib/nextcorrect.py:62-69,193).  `words` is the .2bit
 * payload layout of lib/bseq.c:114-139 (16 bases per uint32, first base in the top two
 * bits); read i starts at words[word_off[i]] and has len[i] bases.  The DB is uploaded to
 * HBM once (forward + reverse complement) and stays there. */
typedef struct ndgpu_db ndgpu_db;
/* NULL when the DB does not fit the device memory */
ndgpu_db *ndgpu_db_create(uint32_t n_reads, const uint32_t *words, const uint64_t *word_off, const uint32_t *len);
/* The same DB from the files the stage already has: `idx_fofn` as given to `nextcorrect.py -f` (one `.NAME.idx` path per line;
 * the `.2bit` next to each is read, as init_ovls() does: lib/ovlseq.c:24-37,50-138).  NULL on I/O / format errors. */
ndgpu_db *ndgpu_db_open(const char *idx_fofn);
void ndgpu_db_destroy(ndgpu_db *db);

/* Correct piles given as overlap records against a resident DB: the batched
 * equivalent of lib/nextcorrect.py:183-199 (worker) + nextCorrect().  `recs` holds
 * 8 uint32 per record in decode_ovl order (lib/ovl.c:189-200, lib/nextcorrect.py:106:
 * seed, rev, t_s, t_e, query read, q_s, q_e, match; coordinates inclusive); pile i owns
 * records [pile_off[i], pile_off[i+1]) and its first record is the seed self record.
 * max_aln_length and the per-pile max_lq_length = min(seed_len/2, max_lq_length) are
 * derived exactly as lib/nextcorrect.py:117,135-137,188 does.  Returns 0; -1 for a dead handle; -2 (nothing computed) when
 * a record names a read that is not in `db` or a window outside its read.  Sub-batches that do not fit the device memory
 * are halved; a single pile that still does not fit comes back as the reference's out-of-memory seed (len 3,
 * lib/nextcorrect.c:2254-2261).  Several handles may be alive; every call works against the one it is given. */
int ndgpu_correct_piles(ndgpu_db *db, int n_piles, const uint32_t *recs, const uint64_t *pile_off,
                        unsigned int min_len_aln, unsigned int max_cov_aln, unsigned int min_cov,
                        unsigned int max_lq_length, float min_error_corrected_ratio, unsigned int split,
                        unsigned int fast, int read_type, int host_threads, consensus_trimed **out);

/* The same call, handing the records over as they become ready: `done(user, pile_ids, n)` is called once per finished sub-batch
 * (n piles whose out[pile_ids[k]] are final), from the host thread that drove that sub-batch, one call at a time (the library
 * serialises them).  The reference streams its records the same way -- the parent of lib/nextcorrect.py:232-260 prints each seed
 * as its worker returns it, in no particular order -- so a caller can write cns.fasta while the later sub-batches are still on the
 * device.  Every pile is reported exactly once before the call returns; done == NULL makes this ndgpu_correct_piles. */
typedef void (*ndgpu_piles_done_fn)(void *user, const uint32_t *pile_ids, int n);
int ndgpu_correct_piles_stream(ndgpu_db *db, int n_piles, const uint32_t *recs, const uint64_t *pile_off,
                               unsigned int min_len_aln, unsigned int max_cov_aln, unsigned int min_cov,
                               unsigned int max_lq_length, float min_error_corrected_ratio, unsigned int split,
                               unsigned int fast, int read_type, int host_threads, consensus_trimed **out,
                               ndgpu_piles_done_fn done, void *user);

/* ndgpu_align_batch (above) over windows of the resident DB. */
int ndgpu_align_db_batch(ndgpu_db *db, const ndgpu_aln_dbjob *jobs, int n, int flags, ndgpu_aln_result *res, uint32_t **cigar,
                         char **q_aln, char **t_aln);

/* Counters accumulated by this process's device runtime since the last reset. */
typedef struct {
    uint64_t tasks, wide_tasks, cells, d_steps, trace_bits, columns, pool_bases, seq_bases;
    uint32_t max_band, forward_launches;
    double forward_ms;      /* HIP-event time of K7 (O(ND) forward) launches */
    double traceback_ms, tags_ms, links_ms, score_ms, extract_ms;
    uint64_t piles, tags, cells_msa, path_items, links, score_launches;
    double backtrack_ms;
    uint64_t score_segments;   /* scoring-DP segments (K10) */
    uint64_t score_repairs;    /* of which scored again after a failed boundary check */
    uint64_t score_slow_piles; /* piles scored by the int64 HBM-resident kernel */
    uint64_t trace_words;      /* 64-bit words of move-bit records K7 wrote (8 bytes per edit step up to 56 cells, 16 beyond) */
    uint64_t lq_rounds;        /* low-quality-region rounds (pile x round) handed to K12 */
    uint64_t lq_declined;      /* of which the kernel declined: the host path took them */
    double lq_ms;              /* HIP-event time of K12 */
    uint64_t allocs;           /* device / pinned buffers (re)allocated while batches were running, since the last reset ... */
    double alloc_ms;           /* ... and the wall time those calls took: an allocation in the middle of a step stalls every context,
                                  so steady-state steps should show none */
    uint64_t level_allocs;     /* the same between batches (buffers brought up to the largest sub-batch seen, nothing in flight) */
    double level_ms;
    uint64_t traceback_launches; /* K8a launches */
    uint64_t lq_launches;      /* K12 launches, and what they moved algorithmically: */
    uint64_t lq_columns;       /* columns of the linked pseudo-seeds walked */
    uint64_t lq_aln_columns;   /* alignment columns (2-bit kinds) read */
    uint64_t lq_bases;         /* candidate bases (2-bit) read */
    uint64_t lq_out;           /* consensus characters written */
    uint64_t lq_jobs;          /* K12 jobs (runs of regions scored from a speculative start) */
    uint64_t lq_repairs;       /* of which scored again after a failed boundary check */
    uint64_t tb_tasks;         /* alignments whose traceback ran in segments (one lane per 2^k edit steps) */
    uint64_t tb_walkers;       /* segments they were cut into */
    uint64_t tb_fallbacks;     /* of the alignments: walked again in one piece (a segment boundary did not agree) */
    uint64_t poa_jobs;         /* POA problems offered to the device (ndgpu_poa_batch, the engine's pseudo-seeds) */
    uint64_t poa_declined;     /* of which declined: the host path took them */
    uint64_t poa_rounds;       /* lockstep rounds: sequence r of every problem that has one */
    uint64_t poa_launches;     /* kernel launches */
    uint64_t poa_cells;        /* (X + 1)(Y + 1) alignment cells filled */
    double poa_ms;             /* HIP-event time of the POA kernels */
    uint64_t rank_jobs;        /* candidate sets ranked on the device (ndgpu_lq_rank_batch, the engine's regions with NDGPU_RANK_DEVICE=1) */
    uint64_t rank_tail;        /* of which took the tail pass */
    uint64_t rank_launches;    /* launches of the ranking kernel */
    double rank_ms;            /* HIP-event time of the ranking kernel */
    uint64_t aln_batch_jobs;     /* jobs through ndgpu_align_batch / ndgpu_align_db_batch with the device tail (not with flags bit 0) */
    uint64_t aln_batch_launches; /* launches of the kernel that writes the runs (one per chunk of jobs that has a run) */
    uint64_t aln_batch_runs;     /* CIGAR runs written on the device */
    double aln_batch_ms;         /* HIP-event time of the run-length kernels (count + emit) */
    uint64_t poa_resident_jobs;     /* POA problems that finished with their graph resident on the device */
    uint64_t poa_resident_declined; /* offered to that path and not finished there (node bound, memory plan, a capacity reached) */
    uint64_t poa_graph_launches;    /* launches of the four graph kernels */
    double poa_graph_ms;            /* their HIP-event time */
    uint64_t poa_h2d_bytes;         /* bytes the POA paths sent to the device */
    uint64_t poa_d2h_bytes;         /* and brought back */
    uint64_t cns_jobs;              /* walks whose consensus words and windows the device made (ndgpu_cns_windows_batch, the engine's piles with NDGPU_CNS_DEVICE=1) */
    uint64_t cns_declined;          /* offered to that kernel and left to the host routine */
    uint64_t cns_launches;          /* its launches */
    uint64_t cns_regions;           /* windows it emitted */
    double cns_ms;                  /* its HIP-event time */
    uint64_t cns_d2h_bytes;         /* result records, words and windows brought back */
    uint64_t walk_d2h_bytes;        /* bytes of main walks (8 per slot of their capacity) the main phase brought back, with or without the kernel */
} ndgpu_stats;
void ndgpu_get_stats(ndgpu_stats *out);
void ndgpu_reset_stats(void);

/* The HiFi and -fast forms of the loop behind the main walk on the device (ndgpu_cns_walk_batch in modes 1 and 2; the engine's piles
 * with NDGPU_CNS_HIFI=1 / NDGPU_CNS_FAST=1).  Counters of their own: ndgpu_stats keeps its layout, its cns_* fields stay the raw-read
 * form's and its walk_d2h_bytes goes on counting every walk that does come down.  ndgpu_reset_stats clears these too. */
typedef struct {
    uint64_t hifi_jobs;             /* HiFi walks the device finished */
    uint64_t hifi_declined;         /* ... offered to the kernel and left to the host routine */
    uint64_t hifi_regions;          /* windows it emitted (a merge emits none) */
    uint64_t fast_jobs;             /* -fast walks the device finished */
    uint64_t fast_declined;
    uint64_t launches;              /* launches of the kernel */
    double ms;                      /* its HIP-event time */
    uint64_t d2h_bytes;             /* result records (32 bytes a walk), words, windows and strings brought back */
} ndgpu_cns_mode_stats;
void ndgpu_get_cns_mode_stats(ndgpu_cns_mode_stats *out);
/* The phasing and ranking of HiFi candidates on the device (ndgpu_hifi_phase_batch; the engine's piles with NDGPU_PHASE_DEVICE=1).
 * Counters of their own: ndgpu_stats keeps its layout.  ndgpu_reset_stats clears these too. */
typedef struct {
    uint64_t piles;                 /* piles the device finished */
    uint64_t regions;               /* their regions ... */
    uint64_t kind[4];               /* ... by kind: empty, dropped, seed, ranked */
    uint64_t pass2_piles;           /* piles whose second pass ran */
    uint64_t tail_passes;           /* ranked regions that took the tail pass */
    uint64_t declined[5];           /* piles left to the host rule: reads over capacity, regions over 65,535, strings outside the pool,
                                       the hook NDGPU_PHASE_DECLINE, a source read out of range */
    uint64_t launches;              /* launches of the kernel pair */
    double ms;                      /* its HIP-event time */
    uint64_t d2h_record_bytes;      /* pile records (32 bytes) and region records (128 bytes) brought back */
    uint64_t d2h_string_bytes;      /* candidate strings brought back beside them (the engine's piles) */
    uint64_t seed_lower;            /* seed regions whose pseudo-seed goes to lower case */
} ndgpu_phase_stats;
void ndgpu_get_phase_stats(ndgpu_phase_stats *out);

/* The splice, its table of lower-case runs and the SSR trim on the device (K24: ndgpu_splice_batch).  Counters of their own:
 * ndgpu_stats keeps its layout.  ndgpu_reset_stats clears these too. */
typedef struct ndgpu_splice_stats {
    uint64_t jobs;        /* jobs offered to the device */
    uint64_t declined;    /* ... of which the host statement answered */
    uint64_t launches;    /* launches of K24 (each with its gather) */
    uint64_t h2d_bytes;   /* records, words and pseudo-seed bytes sent up */
    uint64_t d2h_bytes;   /* result records and result strings brought back */
    uint64_t trimmed;     /* jobs whose gate let the SSR trim run */
    double ms;            /* K24's HIP-event time */
} ndgpu_splice_stats;
void ndgpu_get_splice_stats(ndgpu_splice_stats *out);
/* The device contexts keep their (grow-only) buffers between calls.  This hands them back -- for a caller that alternates
 * the consensus with another memory-hungry stage on the same device (the overlap stage of a genome-scale read set) and
 * finds that stage short of memory.  Safe to call at any time from any thread: a context that is in the middle of a batch
 * (another thread inside nextCorrect / ndgpu_correct_*) keeps its buffers and is skipped.  Returns the bytes released; buffers
 * are re-created on demand. */
uint64_t ndgpu_release_memory(void);
/* Device bytes the consensus contexts must leave free when they size their buffers (the memory plan of every batch call subtracts
 * them from what is free): what another stage on the same device -- the overlap stage of the next seed file -- will need again. */
void ndgpu_reserve_device_memory(uint64_t bytes);
/* Number of HIP devices visible (0 if none); does not create a context. */
int ndgpu_device_count(void);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
