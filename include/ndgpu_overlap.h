/* ndgpu_overlap.h -- C ABI of the MI355X overlap engine (libndgpu_overlap.so).
 *
 * Drop-in scope: the `minimap2-nd --step 1` path of NextDenovo v2.5.2 (all-vs-all raw-read overlap that feeds
 * ovl_sort -> nextcorrect).  Citations are relative to the reference tree.
 *
 *   reference interface                                   this library
 *   ----------------------------------------------------  -------------------------------------------
 *   mm_set_opt()            minimap2/options.c:84-97       ndgpu_ovl_opt_preset()
 *   main.c:190-193 (--step 1), :241,:328 (--dual), :337-343 (-f)   fields of ndgpu_ovl_opt
 *   mm_idx_gen()            minimap2/index.c:351-370       ndgpu_ovl_index_create()   (K1 sketch + K2 sort/group, HBM resident)
 *   mm_idx_cal_max_occ()    minimap2/index.c:170-191       ndgpu_ovl_index_mid_occ()
 *   mm_idx_destroy()        minimap2/index.c:55-79         ndgpu_ovl_index_destroy()
 *   util/ovl_sort.c (whole program, raw reads)               ndgpu_ovl_sort()  (S1 expand, S2 sort, S3 per-seed filter)
 *   mm_map_file() + the step-1 writer  minimap2/map.c:1376-1403, :1296-1304 + encode_ovl() lib/ovl.c:109-150
 *                                                           ndgpu_ovl_map()  (K1, K3 seeds, sort, K4 chain DP, K5 hits; .ovl bytes)
 *
 * Reads are passed exactly as they are stored in NextDenovo's `.2bit` files (lib/bseq.c:114-139): 16 bases per
 * uint32, first base in the two top bits, A=0 C=1 G=2 T=3; word_off[i] = index of read i's first word in `words`.
 * ids[i] is the numeric read name (the reference prints it with "%u" and compares names as strings,
 * map.c:136,1296; this library reproduces that ordering).
 *
 * All functions fail loudly (return NULL / negative and print to stderr) when no HIP device is usable; there
 * is no CPU fallback.
 */
#ifndef NDGPU_OVERLAP_H
#define NDGPU_OVERLAP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif
#pragma GCC visibility push(default) /* the library is built with -fvisibility=hidden: these are its only exports */

typedef struct ndgpu_ovl_opt {
	int32_t k, w, hpc;                  /* mm_idxopt_t::k, ::w, ::flag & MM_I_HPC          (minimap.h) */
	int32_t no_diag, no_dual;           /* MM_F_NO_DIAG, MM_F_NO_DUAL                      (minimap.h:8-9) */
	int32_t min_cnt, min_chain_score;   /* mm_mapopt_t::min_cnt, ::min_chain_score */
	int32_t bw, max_gap;                /* ::bw, ::max_gap */
	int32_t max_chain_skip, max_chain_iter;
	int32_t minlen;                     /* --minlen (500 for --step 1) */
	int32_t seed;                       /* --seed (11) */
	int32_t dvt, maxhan1, maxhan2;      /* --dvt, --maxhan1, --maxhan2 */
	float   mid_occ_frac;               /* -f FLOAT (< 1) */
	int32_t mid_occ;                    /* -f INT (>= 1); 0 = derive from mid_occ_frac */
	int32_t mode;                       /* --mode (2); 3 = HiFi: chain ends trimmed (nd_fix_bad_ends, map.c:340-373) and every hit
	                                       extended into the unaligned read ends (nd_extend_ends, map.c:385-482) before the filter */
	float   d_factor;                   /* --df (0.1): weight of the extension's running score (x + y) * d_factor - d */
	int32_t step;                       /* --step: 1 (raw reads, 8-field records) or 2 (corrected reads, `cns_align`, 10-field records) */
	float   minide;                     /* --step 2: --minide (0.05) */
	int32_t minmatch;                   /* --step 2: --minmatch (100) */
	int32_t max_occ;                    /* -f FLOAT,INT (mm_mapopt_t::max_occ, main.c:343): when > the mid_occ of a map call, a query read
	                                       that chained nothing is seeded again with this threshold and chained again (map.c:553-575,
	                                       :678-700); 0 (every preset) = never */
} ndgpu_ovl_opt;

typedef struct ndgpu_ovl_index ndgpu_ovl_index;

/* one step-1 overlap before varint coding: the fields of `overlap` (lib/ovl.h:20-25) */
typedef struct ndgpu_ovl_rec {
	uint32_t rev, qname, qs, qe, tname, ts, te, match;
} ndgpu_ovl_rec;

/* mm_mapopt_init + mm_idxopt_init + mm_set_opt(preset) + `--step 1`; preset = "ava-ont" | "ava-pb" | "ava-hifi"
 * (options.c:84-111; ava-hifi = k 51, w 51, HPC: the two-word k-mer sketch mm_sketch_nextdenovo_longkmer, sketch.c:283-356).
 * Returns 0, or -1 for an unknown preset.  k may be 1..127 except 32, 64 and 96 (mm_sketch's own range: sketch.c:84, :286-293). */
int ndgpu_ovl_opt_preset(const char *preset, ndgpu_ovl_opt *opt);

/* Sketch the target reads on the device and build the minimizer index in HBM. */
ndgpu_ovl_index *ndgpu_ovl_index_create(const ndgpu_ovl_opt *opt, uint32_t n_reads, const uint32_t *words, uint64_t n_words,
                                        const uint64_t *word_off, const uint32_t *lens, const uint32_t *ids);
void ndgpu_ovl_index_destroy(ndgpu_ovl_index *idx);
/* occurrence threshold of the top `frac` repetitive minimizers (+1), as mm_idx_cal_max_occ */
int32_t ndgpu_ovl_index_mid_occ(ndgpu_ovl_index *idx, float frac);
/* n[0] = minimizers, n[1] = distinct minimizers, n[2] = target reads */
void ndgpu_ovl_index_stat(const ndgpu_ovl_index *idx, uint64_t n[3]);

/* Map the query reads against the index; returns the number of overlaps kept by the step-1 filter
 * (self hits dropped, query span >= minlen, optional --dvt) in reference output order, or < 0 on error.
 * *recs is malloc'd (release with ndgpu_ovl_free). */
int64_t ndgpu_ovl_map(ndgpu_ovl_index *idx, const ndgpu_ovl_opt *opt, int32_t mid_occ, uint32_t n_reads, const uint32_t *words,
                      uint64_t n_words, const uint64_t *word_off, const uint32_t *lens, const uint32_t *ids,
                      ndgpu_ovl_rec **recs);

/* encode_ovl(): append `n` records to a byte buffer as 8 big-endian base-128 varints each;
 * prev[2] = running (qname, tname) state (`prev_t pid`, minimap2/main.c:29).  out needs 40 bytes per record.
 * Returns bytes written. */
int64_t ndgpu_ovl_encode(const ndgpu_ovl_rec *recs, int64_t n, uint32_t prev[2], uint8_t *out);

/* decode_ovl() over a whole buffer (lib/ovl.c:152-203, the routine lib/nextcorrect.py:105 calls per record through ovlseq.so):
 * out[8 * k ..] = qname, rev, qs, qe, tname, ts, te, match of record k; prev[2] = running (qname, tname) state; a trailing
 * partial record is not consumed (*consumed = bytes used, may be NULL).  Returns the records decoded (<= cap). */
int64_t ndgpu_ovl_decode(const uint8_t *buf, uint64_t n_bytes, uint32_t prev[2], uint32_t *out, int64_t cap, uint64_t *consumed);
/* the walk of kbit_read() (lib/bseq.c:257-299) over a .2bit payload without its 2 magic bytes: ids, lengths and the word
 * index of every read's sequence.  Returns the number of reads in the payload (cap = 0: count only), -1 when a record's words
 * run past the payload (truncated / corrupt file). */
int64_t ndgpu_2bit_index(const uint32_t *words, uint64_t n_words, uint32_t *ids, uint32_t *lens, uint64_t *word_off, int64_t cap);

/* ---- read ingestion: the FASTA / FASTQ[.gz] reader of `seq_dump` (util/seq_dump.c:60-118 over kseq_read, util/kseq.h:178-222) ----
 * Streams the file (1 MB inflate window).  ndgpu_fastx_read appends the next records' sequences back to back into buf (cap bytes),
 * off[k] / len[k] = where record k starts / its length, at most max_recs records and never a partial one.  Returns the number of
 * records; 0 = the stream is over (end of file, or the point where kseq_read gives up: a quality string of another length than its
 * sequence); -3 = read error; -4 = the next record alone exceeds cap (ndgpu_fastx_pending = its length; call again with room). */
typedef struct ndgpu_fastx ndgpu_fastx;
ndgpu_fastx *ndgpu_fastx_open(const char *path);
int64_t ndgpu_fastx_read(ndgpu_fastx *h, uint8_t *buf, uint64_t cap, uint64_t *off, uint32_t *len, int64_t max_recs);
/* the same, also handing out strtoul(name) of every record (the numeric read names of the corrected-read files that
 * minimap2-nd --step 2 maps, minimap2/map.c:1298-1300); ids may be NULL */
int64_t ndgpu_fastx_read_named(ndgpu_fastx *h, uint8_t *buf, uint64_t cap, uint64_t *off, uint32_t *len, uint32_t *ids, int64_t max_recs);
uint64_t ndgpu_fastx_pending(const ndgpu_fastx *h);
void ndgpu_fastx_close(ndgpu_fastx *h);
/* The byte stream under ndgpu_fastx, by itself: gzread() (zlib.h; what KSEQ_INIT(gzFile, gzread) reads through, lib/bseq.h:3) with the
 * gzip file inflated by `threads` host threads (0 = NDGPU_INFLATE_THREADS, or the CPUs the process may use, at most 16) -- the same
 * bytes: members concatenated, trailing garbage ignored, a truncated file hands out what it holds, -1 for corrupt data.  With 1
 * thread, or for what is not a regular file starting with a gzip member, the reader IS zlib's.  ndgpu_gzin_stats: 1 and
 * {rounds, chunks decoded, chunks accepted} when the threaded reader is in use, else 0. */
typedef struct ndgpu_gzin ndgpu_gzin;
ndgpu_gzin *ndgpu_gzin_open(const char *path, int threads);
int64_t ndgpu_gzin_read(ndgpu_gzin *h, void *buf, uint32_t len);
int ndgpu_gzin_stats(const ndgpu_gzin *h, uint64_t out[3]);
void ndgpu_gzin_close(ndgpu_gzin *h);

void ndgpu_ovl_free(void *p);
/* Why an entry point of this library failed: 1 = out of device memory (release memory, e.g. ndgpu_ovl_trim() and the consensus
 * library's ndgpu_release_memory(), and call again), 2 = another error of a device operation, 0 = no device operation failed.  Cleared by the call. */
int ndgpu_ovl_last_error(void);
/* The library keeps freed device blocks cached between calls (at most 1.25 x the most it ever had in use at once, and
 * NDGPU_OVL_POOL_GB if set); this releases them.
 * Returns the bytes released. */
uint64_t ndgpu_ovl_trim(void);
/* Declare a host buffer of 2-bit read words (the `words` array of the calls below, as stored in a .2bit file) resident: it is uploaded once,
 * and every later call whose `words` lie inside it works on the device copy instead of uploading them again (index build and query side of
 * every raw_align job name the same reads).  The buffer must stay valid and unchanged until ndgpu_ovl_words_release().  Additive: the
 * reference has no counterpart (its reads live in host memory, lib/bseq.c).  Returns 0, -1 on failure (out of device memory). */
int ndgpu_ovl_words_resident(const uint32_t *words, uint64_t n_words);
void ndgpu_ovl_words_release(const uint32_t *words);
/* out[0] = device bytes the library has in use now, out[1] = cached for reuse, out[2] = the most it ever had in use at once -- what a
 * caller that runs another memory-hungry stage on the same device between two calls should leave free (out[2] - out[1]). */
void ndgpu_ovl_pool_bytes(uint64_t out[3]);
/* out[0] = hipMalloc / hipFree calls the library's block pool has made, out[1] = nanoseconds they took (such a call stalls every stream
 * of the process, the consensus contexts' included); reset != 0 clears the counters */
void ndgpu_ovl_pool_calls(uint64_t out[2], int reset);

/* ---- overlap sort / filter: the `ovl_sort` program between the two stages (util/ovl_sort.c, raw reads, no -H) ----
 *
 *   files[f][0..n_per_file[f])  step-1 records of input file f in file order (what ndgpu_ovl_map returned, or a decoded .ovl:
 *                               half-open ends), files in input.fofn order
 *   seed_len[id]                length of read `id` if it is a seed of this seed file (its .idx, util/ovl_sort.c:106-131), else 0
 *   min_seed_len                shortest seed of the .idx;  max_bin_cov = -k (40);  max_flank_len = -l (300)
 *
 * Returns the records of `sorted.ovl` in file order (per seed: the self record, then the admitted overlaps, inclusive
 * ends; util/ovl_sort.c:675-741, 433-571, 876-925) and the `.bl` verdicts ('c' contained, 'k' chimeric) in seed order.
 * Equal (seed, match, span) keys keep input order.  When the candidates do not fit the device at once (~360 bytes per raw record all
 * told) the raw records -- which stay in the caller's arrays -- pass the device twice in pieces and the seeds are sorted and filtered
 * in consecutive id ranges (the counterpart of the reference's temporary files and merge under a small -m, util/ovl_sort.c:1079-1110:
 * like there, the result is the same); NDGPU_OVLSORT_PIECE_RECORDS / NDGPU_OVLSORT_RANGE_CANDIDATES force that form.
 * All three outputs are malloc'd (ndgpu_ovl_free). */
typedef struct ndgpu_ovl_sort_stats { double gpu_ms; uint64_t raw_records, candidates, seeds, kept, ranges; } ndgpu_ovl_sort_stats;  /* ranges: seed-id ranges the candidates were sorted in (1 = all at once) */
int64_t ndgpu_ovl_sort(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                       uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, ndgpu_ovl_rec **out,
                       uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats);
/* the same with `-H` (high-quality reads, util/ovl_sort.c:27,1045): every candidate is collected, overlaps that start and end at hot
 * break points (del_repeat_alns, :389-431) are dropped, chimeras come from uncovered bins no overlap spans (check_chimer_hq,
 * :287-314), a containing overlap counts only with >= 90 % matches (:555) */
int64_t ndgpu_ovl_sort_hq(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                          uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, ndgpu_ovl_rec **out,
                          uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats);

/* ---- pile admission between the sort and the consensus: read_seq_data of lib/nextcorrect.py:92-143 on the records of a sorted.ovl
 * (what ndgpu_ovl_sort returned).  One pile per seed whose length is >= min_len_seed and that is not in skip_ids (the `.bl` list /
 * seeds already corrected): overlaps shorter than min_len_aln, repeated query reads and overlaps beyond 1.5 x max_cov_aln of
 * cumulative depth are dropped, piles below min_cov_seed of depth are dropped.  recs8[i] = the admitted record i in the field order
 * nextCorrect's callers use (seed, rev, seed start, seed end (inclusive), read, read start, read end, match); pile p =
 * recs8[pile_off[p] .. pile_off[p+1]); seeds[p] = its seed id.  Host logic (no device work); outputs malloc'd (ndgpu_ovl_free).
 * Returns the number of admitted records. */
int64_t ndgpu_assemble_piles(const ndgpu_ovl_rec *sorted, int64_t n, uint32_t n_ids, uint32_t min_len_seed, uint32_t min_len_aln,
                             uint32_t max_cov_aln, uint32_t min_cov_seed, const uint32_t *skip_ids, int64_t n_skip, uint32_t **recs8,
                             uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles);

/* ---- the same admission on the device (K16, one wavefront per seed group; csrc/ovlsort_kernels.hip) ----
 * On a well-formed stream -- every group of records with one seed id starts with a record the loop admits or with one that rejects
 * the whole group -- the loop's verdicts are a per-group rule with one prefix sum, and the device applies it.  A group where the
 * loop's last_seed / '+' state would split the group again is "irregular": a valid seed whose first record is shorter than
 * min_len_aln, a rejected seed with a later record that passes as a seed, t_e < t_s, a query id >= n_ids.  One such group and the
 * whole call is answered by ndgpu_assemble_piles (groups_declined says so); ndgpu_ovl_sort's output is regular at nextDenovo's
 * thresholds.  The result is ndgpu_assemble_piles's either way.
 *   sorted_records    records the admission saw;  groups = seed groups among them
 *   groups_declined   irregular groups found before the call turned to the host routine (0: the device's answer)
 *   groups_wide       groups whose table of seen query reads did not fit LDS (more than 1024 records, or more than half of
 *                     NDGPU_ADMIT_TABLE=<slots>, which forces a smaller table) and lived in global memory
 *   admitted, piles   records and piles handed out
 *   k16_ms            HIP-event time of the admission tail: the two kernel passes, the scans between them, the downloads
 *   bytes_downloaded  bytes copied from the device for the call's outputs (rows, offsets, seeds, `.bl` lists, sorted records if any) */
typedef struct ndgpu_ovl_admit_stats {
	double k16_ms;
	uint64_t sorted_records, groups, groups_declined, groups_wide, admitted, piles, bytes_downloaded;
} ndgpu_ovl_admit_stats;
/* array-level view: the arguments and the three blocks of ndgpu_assemble_piles; the records are uploaded, K16 runs, only what was
 * admitted comes back.  flags bit 0: the host routine instead (a cross-check); bit 1 reserved (0).  stats may be NULL.
 * n = 0 and "every seed rejected" give pile_off = {0}.  Returns the number of admitted records; -1 no device, -2 a device operation
 * failed (ndgpu_ovl_last_error), -3 more than 2^30 records. */
int64_t ndgpu_admit_piles(const ndgpu_ovl_rec *sorted, int64_t n, uint32_t n_ids, uint32_t min_len_seed, uint32_t min_len_aln,
                          uint32_t max_cov_aln, uint32_t min_cov_seed, const uint32_t *skip_ids, int64_t n_skip, int32_t flags,
                          uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles, ndgpu_ovl_admit_stats *stats);
/* ndgpu_ovl_sort (hq != 0: ndgpu_ovl_sort_hq) with the admission as its tail: the sorted records, their group offsets and the
 * `.bl` verdicts are admitted where the sort left them, range by range in the out-of-core form.  The skip set is skip_ids plus,
 * with use_bl != 0, the seeds of this sort's own `.bl` verdicts.  Only recs8 / pile_off / seeds and the `.bl` lists are downloaded;
 * the sorted records too when `sorted` is not NULL (*sorted malloc'd, *n_sorted records) -- or when a group declined, for the host
 * routine.  flags as above.  Everything handed out is malloc'd (ndgpu_ovl_free).  Returns the number of admitted records, or
 * ndgpu_ovl_sort's error codes. */
int64_t ndgpu_ovl_sort_piles(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                             uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq,
                             uint32_t min_len_seed, uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, int32_t use_bl,
                             const uint32_t *skip_ids, int64_t n_skip, int32_t flags, uint32_t **bl_id, uint8_t **bl_kind,
                             int64_t *n_bl, uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                             ndgpu_ovl_rec **sorted, int64_t *n_sorted, ndgpu_ovl_sort_stats *stats, ndgpu_ovl_admit_stats *astats);

/* ---- the `.ovl` codec on the device (K17; csrc/ovlsort_kernels.hip): what ndgpu_ovl_encode / ndgpu_ovl_decode do, as scans ----
 * A value of the host loop, v = (v << 7) | (c & 127) in 32 bits, depends on its terminator and the 4 bytes in front of it only, so
 * the device form equals the loop on every byte string: nothing declines.  Decode: terminators counted per 16 bytes, a prefix gives
 * every value its index, value j of a file = field j % 8 of record j / 8, the names are prefix sums of the signed deltas modulo 2^32,
 * restarted per file.  Encode: one lane per record, sizes, a prefix, the bytes staged per wavefront and stored once.
 *   decode_ms, encode_ms             HIP-event time of the decode (image upload -- with the page faults of a memory-mapped file --, kernels, scans)
 *                                    and of the encode (kernels, scan)
 *   records                          records decoded / encoded
 *   bytes_in, bytes_out              size of what the call was given and of what it made (images or 32-byte records)
 *   bytes_uploaded, bytes_downloaded `.ovl` images and records copied to / from the device (not the few control words)
 *   host_decodes                     files the host loop decoded (flags bit 0, a sort in seed ranges, a declined admission) */
typedef struct ndgpu_ovl_codec_stats {
	double decode_ms, encode_ms;
	uint64_t records, bytes_in, bytes_out, bytes_uploaded, bytes_downloaded, host_decodes;
} ndgpu_ovl_codec_stats;
/* n_files images (bufs[f], n_bytes[f]) -> all their records in one malloc'd block (ndgpu_ovl_free), file after file; every file
 * starts from prev = {0, 0}.  n_per_file[f] = its whole records, consumed[f] (may be NULL) = the offset behind the last of them (a
 * trailing partial record is left alone, as by ndgpu_ovl_decode).  flags bit 0: the host loop per file.  stats may be NULL.
 * Returns the number of records; -1 no device, -2 a device operation failed (ndgpu_ovl_last_error), -4 a bad argument.  On an
 * error *recs stays NULL and nothing else is written. */
int64_t ndgpu_ovl_decode_batch(const uint8_t *const *bufs, const uint64_t *n_bytes, int32_t n_files, int32_t flags, ndgpu_ovl_rec **recs,
                               int64_t *n_per_file, uint64_t *consumed, ndgpu_ovl_codec_stats *stats);
/* ndgpu_ovl_encode with the output allocated: *out = the bytes, malloc'd at their exact size (ndgpu_ovl_free); prev[2] is read and
 * updated as there.  flags bit 0: the host loop.  Returns the byte count, or an error code as above (prev untouched, *out NULL). */
int64_t ndgpu_ovl_encode_batch(const ndgpu_ovl_rec *recs, int64_t n, uint32_t prev[2], int32_t flags, uint8_t **out,
                               ndgpu_ovl_codec_stats *stats);
/* The `ovl_sort` command in one device pass: the step-1 files as images in, the image of `sorted.ovl` and the `.bl` verdicts out
 * (hq != 0: the -H filter).  The images are decoded into the sort's own buffer and every seed range's sorted records are encoded
 * where they lie, `prev` carried from range to range: no 32-byte record crosses the bus.  A sort in seed ranges (see ndgpu_ovl_sort)
 * reads its files from host memory: they are decoded by the host loop (codec_stats->host_decodes), the ranges still encoded on the
 * device.  flags bit 0: host decode, ndgpu_ovl_sort, host encode.  Everything handed out is malloc'd (ndgpu_ovl_free).  Returns the
 * number of sorted records, ndgpu_ovl_sort's error codes, or -4 for a bad argument. */
int64_t ndgpu_ovl_sort_images(const uint8_t *const *bufs, const uint64_t *n_bytes, int32_t n_files, const uint32_t *seed_len, uint32_t n_ids,
                              int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq, int32_t flags, uint8_t **image,
                              uint64_t *image_bytes, uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *sort_stats,
                              ndgpu_ovl_codec_stats *codec_stats);
/* ndgpu_admit_piles on the image of a sorted.ovl: the bytes are uploaded and decoded on the device, K16 admits the records.  A stream
 * with an irregular group (admit_stats->groups_declined) is decoded by the host loop and answered by ndgpu_assemble_piles, as is
 * flags bit 0.  Returns the number of admitted records, or the error codes of ndgpu_admit_piles, -4 for a bad argument. */
int64_t ndgpu_admit_piles_image(const uint8_t *buf, uint64_t n_bytes, uint32_t n_ids, uint32_t min_len_seed, uint32_t min_len_aln,
                                uint32_t max_cov_aln, uint32_t min_cov_seed, const uint32_t *skip_ids, int64_t n_skip, int32_t flags,
                                uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                                ndgpu_ovl_admit_stats *admit_stats, ndgpu_ovl_codec_stats *codec_stats);

/* ---- record sets: the step-1 records of a job, wherever they are (K18; csrc/ovlsort_kernels.hip) ----
 * A set holds n records in device memory of the library's block pool, in the order ndgpu_ovl_map returns them.  It is read-only once
 * made; any number of sort calls may read it (the `ln -sf` mirror of a seed x seed job, nextDenovo:459, is one set read by the sorts
 * of two seed files), from any thread.  A set is live pool memory until it is freed: ndgpu_ovl_trim does not touch it and
 * ndgpu_ovl_pool_bytes counts it as in use.  The calls that make a set return it through their last argument, or NULL with the
 * error codes -1 (no device) and -2 (a device operation failed: ndgpu_ovl_last_error; what was made so far is freed). */
typedef struct ndgpu_ovl_recset ndgpu_ovl_recset;
/* ndgpu_ovl_map with the records left on the device: same arguments, same return value, *set instead of *recs (an empty query set
 * gives 0 and an empty set).  Every batch's records are appended device to device in read order; the call returns with the index's
 * stream synchronised, so a consumer on another stream needs no event.  The 8-field records only (--mode 3 included): opt->step == 2
 * is refused with -1. */
int64_t ndgpu_ovl_map_dev(ndgpu_ovl_index *idx, const ndgpu_ovl_opt *opt, int32_t mid_occ, uint32_t n_reads, const uint32_t *words,
                          uint64_t n_words, const uint64_t *word_off, const uint32_t *lens, const uint32_t *ids, ndgpu_ovl_recset **set);
/* records in a set (0 for NULL) */
int64_t ndgpu_ovl_recset_size(const ndgpu_ovl_recset *set);
/* the records of a set to out[0 .. cap): returns their number, -4 when cap is smaller, -2 when the copy failed */
int64_t ndgpu_ovl_recset_download(const ndgpu_ovl_recset *set, ndgpu_ovl_rec *out, int64_t cap);
/* a set made from n host records (what another rank handed over arrives on the host); NULL on failure (ndgpu_ovl_last_error) */
ndgpu_ovl_recset *ndgpu_ovl_recset_upload(const ndgpu_ovl_rec *recs, int64_t n);
/* a new set: the n inputs back to back, copied device to device (the -I parts of one target, part-major); the inputs stay as they
 * are.  NULL on failure. */
ndgpu_ovl_recset *ndgpu_ovl_recset_concat(const ndgpu_ovl_recset *const *sets, int32_t n);
/* K18, the stable split: out_sets[f] (n_files entries) = the records of `set` whose file_of[qname] == f, in their order in `set` --
 * what a stable argsort by file and a cut at the file boundaries give on the host.  file_of has n_ids entries, < n_files each.  Two
 * passes over the records (count per 512-record tile and file, one scan, scatter): no atomics on the output positions, so the order
 * does not depend on how the device schedules lanes and wavefronts.  The output sets share one buffer, released with the last of
 * them.  Returns 0; -1 no device; -2 a record's qname >= n_ids or its file_of entry is 0xffffffff (or a device operation failed:
 * ndgpu_ovl_last_error != 0) -- no set is made; -4 a bad argument or n_files > 256 (the caller cuts on the host). */
int64_t ndgpu_ovl_recset_split(const ndgpu_ovl_recset *set, const uint32_t *file_of, uint32_t n_ids, int32_t n_files,
                               ndgpu_ovl_recset **out_sets);
/* NULL is fine */
void ndgpu_ovl_recset_free(ndgpu_ovl_recset *set);
/* ndgpu_ovl_sort (hq != 0: ndgpu_ovl_sort_hq) and ndgpu_ovl_sort_piles with the input files as sets: every other argument, output and
 * stats structure is theirs.  The records reach the sort's buffer by device-to-device copies and the file of every record is filled in
 * on the device.  A sort in seed ranges (see ndgpu_ovl_sort) reads its files from host memory twice: for it the sets are downloaded
 * once into buffers the call owns (counted in sets_downloaded).  Nothing is refused that the host-records calls accept. */
int64_t ndgpu_ovl_sort_sets(const ndgpu_ovl_recset *const *files, int32_t n_files, const uint32_t *seed_len, uint32_t n_ids,
                            int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq, ndgpu_ovl_rec **out,
                            uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats);
int64_t ndgpu_ovl_sort_piles_sets(const ndgpu_ovl_recset *const *files, int32_t n_files, const uint32_t *seed_len, uint32_t n_ids,
                                  int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq, uint32_t min_len_seed,
                                  uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, int32_t use_bl,
                                  const uint32_t *skip_ids, int64_t n_skip, int32_t flags, uint32_t **bl_id, uint8_t **bl_kind,
                                  int64_t *n_bl, uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                                  ndgpu_ovl_rec **sorted, int64_t *n_sorted, ndgpu_ovl_sort_stats *stats, ndgpu_ovl_admit_stats *astats);
/* counters of the process since the last reset (sets_live is never reset):
 *   split_ms                          HIP-event time of the split calls (two kernel passes, the scan, the cut points' download)
 *   sets_made, sets_live              sets handed out; sets not freed yet
 *   bytes_downloaded, bytes_uploaded  record bytes copied to / from the host on behalf of sets (download, upload, a sort in seed ranges)
 *   bytes_d2d                         record bytes copied device to device (map batches, concat, split, the sorts' input)
 *   split_calls                       ndgpu_ovl_recset_split calls that ran
 *   sets_downloaded                   sets a sort in seed ranges had to download */
typedef struct ndgpu_ovl_recset_counters {
	double split_ms;
	uint64_t sets_made, sets_live, bytes_downloaded, bytes_uploaded, bytes_d2d, split_calls, sets_downloaded;
} ndgpu_ovl_recset_counters;
void ndgpu_ovl_recset_stats(ndgpu_ovl_recset_counters *out, int reset);

/* ---- read ingestion: the 2-bit packing of `seq_dump` (seq2bit, lib/bseq.c:114-139; called from util/seq_dump.c:36-41) ----
 * Read i is the lens[i] ASCII bytes at ascii + ascii_off[i]; its ceil(lens[i]/16) words go to words + word_off[i] (word_off ascending,
 * reads back to back).  Bytes other than ACGTU (either case) are coded 4 and OR-ed in as the reference does, so they disturb the low
 * bit of the preceding base.  Returns the number of words written, < 0 on error. */
int64_t ndgpu_pack_2bit(uint32_t n_reads, const uint8_t *ascii, uint64_t n_bytes, const uint64_t *ascii_off, const uint32_t *lens,
                        const uint64_t *word_off, uint32_t *words);

/* ---- array-level views used by the parity tests (same library, same kernels) ---- */

/* K1 alone: minimizers of every read; rid_is_index != 0 puts the read index in the high word of y (index
 * side), 0 leaves it 0 (query side, map.c:71).  off[n_reads+1], x/y malloc'd. */
int64_t ndgpu_ovl_sketch(const ndgpu_ovl_opt *opt, uint32_t n_reads, const uint32_t *words, uint64_t n_words,
                         const uint64_t *word_off, const uint32_t *lens, int rid_is_index, uint64_t **x, uint64_t **y,
                         uint64_t *off);
/* index arrays: key[n_keys] ascending, start[n_keys+1], pos[n_min] */
void ndgpu_ovl_index_dump(const ndgpu_ovl_index *idx, uint64_t *key, uint64_t *start, uint64_t *pos);
/* after ndgpu_ovl_map(..): the last batch's sorted anchors and chain-DP arrays of query `q` (index into that
 * call's reads).  Returns the anchor count; arrays malloc'd. */
int64_t ndgpu_ovl_debug_anchors(ndgpu_ovl_index *idx, uint32_t q, uint64_t **ax, uint64_t **ay, int32_t **f, int32_t **p);

/* kernel timing of the calls so far on this index (ms, HIP events) and work counters */
typedef struct ndgpu_ovl_stats {
	double sketch_ms, index_sort_ms, seed_ms, sort_ms, exact_sort_ms, chain_ms, hits_ms;
	uint64_t bases_sketched, minimizers, anchors, tie_reads, chain_cells, chains, overlaps, map_calls, batches;
	uint64_t ext_problems, ext_launches; /* --mode 3: end extensions run (two candidates per hit), launches they took */
	double ext_ms;
	uint64_t rechained;                  /* -f FLOAT,INT: query reads seeded and chained a second time */
} ndgpu_ovl_stats;
/* ---- `minimap2-nd --step 2 --mode 0` (the cns_align command of nextDenovo:356-366 with the re-alignment switched off) ----
 * one --step 2 overlap before varint coding: the fields of `overlap_i` (lib/ovl.h); identity = matches * 10000 / block length */
typedef struct ndgpu_ovl_rec10 {
	uint32_t rev, qname, qs, qe, qlen, tname, ts, te, tlen, identity;
} ndgpu_ovl_rec10;
/* replaces: worker_for without re-alignment + the writer's record filter (minimap2/map.c:988-1031, 1305-1309) for the reads of one
 * query file against one index part: hits marked per target, filtered by length / identity / minimum block length.  opt->step must
 * be 2 and opt->mode 0.  *recs is malloc'd (ndgpu_ovl_free).  Returns the record count, < 0 on error. */
int64_t ndgpu_ovl_map2(ndgpu_ovl_index *idx, const ndgpu_ovl_opt *opt, int32_t mid_occ, uint32_t n_reads, const uint32_t *words,
                       uint64_t n_words, const uint64_t *word_off, const uint32_t *lens, const uint32_t *ids, ndgpu_ovl_rec10 **recs);
/* The hits of every query read with nothing judged or filtered, in hit order (mm_map_frag's, minimap2/map.c:506-623): rev, qs, qe,
 * ts, te as usual; `qname` = the hit's target -- its index-local read number, or, with a wanted list, its POSITION in the read's list
 * want[want_off[i] .. want_off[i + 1]) (the read is then mapped against those reads only, which are seen in list order: the
 * per-thread mini-index of the re-alignment, minimap2/index.c:434-575); `tname` = block length, `match` = match count.
 * nameless bit 0: the reads have no names (mm_map(..., qname = 0)): no name-based seed skipping, no self test; bit 1: the chaining
 * is mm_chain_dp_nextdenovo (mm_map_nextdenovo1, minimap2/map.c:1047: a mapping with more than 100,000 anchors is thinned first).  counts[i] = hits
 * of read i; *max_anchors (may be NULL) = the most anchors any one read had.  Both arrays malloc'd (ndgpu_ovl_free).  Returns the
 * number of hits, < 0 on error. */
int64_t ndgpu_ovl_map_regs(ndgpu_ovl_index *idx, const ndgpu_ovl_opt *opt, int32_t mid_occ, uint32_t n_reads, const uint32_t *words,
                           uint64_t n_words, const uint64_t *word_off, const uint32_t *lens, const uint32_t *ids, const uint64_t *want_off,
                           const uint32_t *want, int nameless, ndgpu_ovl_rec **recs, uint32_t **counts, uint64_t *max_anchors);
/* replaces: worker_for WITH the re-alignment (minimap2/map.c:988-1126) + the writer's record filter (:1305-1309): `--step 2` as
 * nextDenovo runs it (no --mode, i.e. --mode 2, options.c:56), or --mode 1 (the two forms of the re-alignment switch at 20 candidates
 * instead of 200, and the one-read-index mappings chain through mm_chain_dp_nextdenovo: a mapping with more than 100,000 anchors
 * loses the anchors of crowded target positions first, chain.c:185-226).  idx = the index part (the preset's k, w); q_mini / t_mini = indexes
 * with the short sketch (--kn 17 --wn 10, main.c:197) over the query reads / over the part's target reads; cn = --cn (20).
 * opt->step must be 2 and opt->mode 1 or 2.  *recs is malloc'd (ndgpu_ovl_free).  Returns the record count, < 0 on error. */
int64_t ndgpu_ovl_map2_realign(ndgpu_ovl_index *idx, ndgpu_ovl_index *q_mini, ndgpu_ovl_index *t_mini, const ndgpu_ovl_opt *opt,
                               int32_t mid_occ, int32_t cn, uint32_t n_t, const uint32_t *t_words, uint64_t t_n_words,
                               const uint64_t *t_word_off, const uint32_t *t_lens, const uint32_t *t_ids, uint32_t n_q,
                               const uint32_t *q_words, uint64_t q_n_words, const uint64_t *q_word_off, const uint32_t *q_lens,
                               const uint32_t *q_ids, ndgpu_ovl_rec10 **recs);
/* replaces: filter_ovl (lib/ovl.c:449-563), whose per-read state lives for the whole run (opt.os, main.c:272), encode_ovl_i
 * (lib/ovl.c:205-253) and out_bl (lib/ovl.c:339-362).  The state is host memory.  A record's verdict depends on the records before it
 * only through "has this read looked contained twice yet": the host loop walks the records in order, K23 (opt-in, below) computes
 * the same verdicts, bytes and per-read state on the device without such a walk. */
typedef struct ndgpu_s2_state ndgpu_s2_state;
ndgpu_s2_state *ndgpu_s2_new(void);
void ndgpu_s2_free(ndgpu_s2_state *st);
/* the records of one ndgpu_ovl_map2 call, in order: verdicts (kept[i], may be NULL) and the bytes of the kept ones (*out, malloc'd,
 * ndgpu_ovl_free); prev[2] is the encoder's delta state, carried from call to call (start: 0, 0).  The file starts with the two
 * bytes 00 FF (init_ovl_mode, lib/ovl.c:70-75), the caller's to write.  Returns the byte count, < 0 on error. */
int64_t ndgpu_s2_filter_encode(ndgpu_s2_state *st, const ndgpu_ovl_rec10 *recs, int64_t n, int32_t maxhan1, int32_t maxhan2,
                               uint32_t prev[2], uint8_t **out, uint8_t *kept);
/* ndgpu_s2_filter_encode with a choice of path; that call is this one with flags 0.
 *   bit 0: the host loop;  bit 1: the device (K23).
 *   Neither: NDGPU_S2_DEVICE=1 in the environment, read at each call, selects bit 1.
 *   Both, or any other bit: -2, nothing written.
 * Verdicts, bytes, prev[] and the later .bl text are the same on every path.  A device call the kernels cannot compute as the
 * reference does -- a query or target span under 21 bases, an identity above 32,767, a read whose 16-bit end counter would reach
 * its limit, no fixed point within NDGPU_S2_MAX_ROUNDS (16) rounds, 2^31 records or more, no device or no device memory,
 * NDGPU_S2_DECLINE=1 -- runs through the host loop on the untouched state and is counted in `declined`.  Host and device calls may
 * alternate on one state. */
int64_t ndgpu_s2_filter_encode_flags(ndgpu_s2_state *st, const ndgpu_ovl_rec10 *recs, int64_t n, int32_t maxhan1, int32_t maxhan2,
                                     uint32_t prev[2], int flags, uint8_t **out, uint8_t *kept);
/* counters of the process since the last reset: calls, records in, records kept, calls the device computed; `declined` by reason;
 * rounds of the fixed point (all device calls, the most of one call); distinct reads of the device calls; merged intervals
 * downloaded; bytes to and from the device; kernel and primitive launches; device time of the calls */
typedef struct ndgpu_s2_stats {
	uint64_t calls, records, kept, device_calls;
	uint64_t declined[6];      /* short span, identity, counter at its limit, rounds, memory / size, the hook */
	uint64_t rounds, max_rounds, reads_touched, spans_down, bytes_up, bytes_down, launches;
	double ms;                 /* HIP events */
} ndgpu_s2_stats;
void ndgpu_s2_get_stats(ndgpu_s2_stats *out);
void ndgpu_s2_reset_stats(void);
/* the `.bl` text written when the run ends (*text malloc'd, ndgpu_ovl_free); the state is spent afterwards */
int64_t ndgpu_s2_bl(ndgpu_s2_state *st, char **text);

/* ---- the base-level extension kernel of minimap2's -c / -a path (off the default correction path: `minimap2-nd --step 1` runs
 *      without -c) ----
 * replaces: ksw_extz_t (minimap2/ksw2.h:23-32), same layout */
typedef struct ndgpu_ksw_extz {
	uint32_t max:31, zdropped:1;
	int max_q, max_t;      /* max extension coordinate */
	int mqe, mqe_t;        /* max score when reaching the end of query */
	int mte, mte_q;        /* max score when reaching the end of target */
	int score;             /* max score reaching both ends; may be KSW_NEG_INF (-0x40000000) */
	int m_cigar, n_cigar;
	int reach_end;
	uint32_t *cigar;
} ndgpu_ksw_extz;
/* replaces: ksw_extd2_sse (minimap2/ksw2.h:60-61, minimap2/ksw2_extd2_sse.c:26-399; caller mm_align_pair, minimap2/align.c:331):
 * global / extension alignment with the two-piece affine gap cost min(gapo + k * gape, gapo2 + k * gape2), band w, z-drop, the
 * KSW_EZ_* flags (score only, right-aligned gaps, generic matrix, approximate maximum / z-drop, extension only, reversed CIGAR).
 * Sequences are codes < m; mat is m x m.  Every field of *ez and the CIGAR are what the reference computes.  km is ignored;
 * ez->cigar is malloc'd (as the reference does with km == NULL) and replaces a buffer the caller passed in. */
void ksw_extd2_sse(void *km, int qlen, const uint8_t *query, int tlen, const uint8_t *target, int8_t m, const int8_t *mat, int8_t gapo,
                   int8_t gape, int8_t gapo2, int8_t gape2, int w, int zdrop, int end_bonus, int flag, ndgpu_ksw_extz *ez);
/* additive: a batch of such problems in one launch, one wavefront per problem (the gaps between the anchors of the chains of a
 * batch of reads, their end extensions).  res[i].cigar is malloc'd (free) when n_cigar > 0.  Returns 0, < 0 on error. */
typedef struct ndgpu_ksw_job {
	const uint8_t *query, *target;
	const int8_t *mat;
	int32_t qlen, tlen, w, zdrop, end_bonus, flag;
	int8_t m, gapo, gape, gapo2, gape2;
} ndgpu_ksw_job;
typedef struct ndgpu_ksw_result {
	int32_t max, zdropped, max_q, max_t, mqe, mqe_t, mte, mte_q, score, n_cigar, reach_end;
	uint32_t *cigar;
} ndgpu_ksw_result;
int ndgpu_ksw_extd2_batch(const ndgpu_ksw_job *jobs, int n, ndgpu_ksw_result *res);

/* replaces: ksw_ll_qinit(km, 2, qlen, query, 5, mat) + ksw_ll_i16 (minimap2/ksw2_ll_sse.c:32-156; callers mm_test_zdrop and
 * mm_align1_inv, minimap2/align.c:80-82,813-815): the striped local-alignment SCORE of a batch of problems, one wavefront each, with
 * the values of the SSE schedule (score, query end, target end -- also for equal maxima and the padding columns).  mat is 5 x 5,
 * codes <= 4.  Returns 0, < 0 on error. */
typedef struct ndgpu_ll_job { const uint8_t *query, *target; const int8_t *mat; int32_t qlen, tlen, gapo, gape; } ndgpu_ll_job;
typedef struct ndgpu_ll_result { int32_t score, qe, te; } ndgpu_ll_result;
int ndgpu_ksw_ll_batch(const ndgpu_ll_job *jobs, int n, ndgpu_ll_result *res);

/* ---- `minimap2-nd --step 1 -c`: base-level alignment through the chains (off the default correction path: nextDenovo runs
 *      --step 1 without -c) ----
 * the scoring side of mm_mapopt_t (minimap.h; defaults mm_mapopt_init, minimap2/options.c:36-43; -A -B -O -E -z -s of main.c) */
typedef struct ndgpu_ovl_aln_opt {
	int32_t a, b, q, e, q2, e2, sc_ambi;  /* match, mismatch, gap open / extend of the two pieces, score of a base against N */
	int32_t zdrop, zdrop_inv, end_bonus;
	int32_t min_dp_max;                   /* -s: 80 (min_chain_score * a when mm_mapopt_init runs; the ava presets do not touch it) */
	int32_t min_ksw_len;                  /* 200: anchors closer than this on either read are bridged by the next gap's alignment */
	int64_t max_sw_mat;                   /* --cap-sw-mem; 0 = none (the default: mm_mapopt_init leaves it 0): a problem of more cells counts as
	                                         z-dropped without being aligned (mm_align_pair, minimap2/align.c:323; the compiled reference segfaults on the first such gap of a
	                                         chain that has no CIGAR yet, so there is nothing to compare a cap with) */
	int32_t host_threads;                 /* threads of the bookkeeping between the batches; 0 = all */
} ndgpu_ovl_aln_opt;
void ndgpu_ovl_aln_opt_default(ndgpu_ovl_aln_opt *o, int32_t min_chain_score);
typedef struct ndgpu_ovl_cigar_stats {
	uint64_t chains, first_pass, second_pass, inversion_tests, inversions, cells, overlaps, inversions_aligned, splits;
	uint64_t chains_ns, ksw_ns, ksw_ll_ns, total_ns;
	/* wall time of the call: sketch / seeds / chaining on the device (ndgpu_ovl_map_chains); the ksw_extd2 batches (upload, kernel,
	 * backtrack, download); the ksw_ll batches; everything (the rest is the host's chain walking, CIGAR joining and filters) */
	/* chains aligned (pieces of split chains included); extension / gap problems of the first pass; gaps aligned again after a
	 * z-drop; local alignments of the inversion test; inversions looked at (mm_align1_inv calls); DP cells (query x target) of all
	 * problems; records out; inversions that were aligned; chains a z-drop split */
} ndgpu_ovl_cigar_stats;
/* array-level view (and the first half of ndgpu_ovl_map_cigar): the chains of every query read as mm_align_skeleton takes them
 * (minimap2/hit.c:52-85): chains[] in hit order, self hits included, = (strand, index-local target, offset of the first anchor in
 * the read's anchors, anchor count, chain score, hash, 0, 0); counts[i] = chains of read i; the chained anchors of read i =
 * ax / ay[a_off[i] .. a_off[i + 1]) in the order of the reference's a[].  Everything malloc'd (ndgpu_ovl_free). */
int64_t ndgpu_ovl_map_chains(ndgpu_ovl_index *idx, const ndgpu_ovl_opt *opt, int32_t mid_occ, uint32_t n_reads, const uint32_t *words,
                             uint64_t n_words, const uint64_t *word_off, const uint32_t *lens, const uint32_t *ids, ndgpu_ovl_rec **chains,
                             uint32_t **counts, uint64_t **ax, uint64_t **ay, uint64_t **a_off);
/* replaces: mm_map_file() + the step-1 writer WITH MM_F_CIGAR: mm_align_skeleton (minimap2/align.c:857-913: mm_align1 per chain --
 * left extension, gap filling with the approximate-then-exact z-drop passes, right extension --, z-drop splits, mm_align1_inv,
 * mm_filter_regs, mm_hit_sort) between chaining and the writer's filter (minimap2/map.c:484-503, 1297-1304).  The records carry the
 * alignments' coordinates and exact match counts.  t_words / t_word_off / t_lens / t_ids = the reads the index was built from (the
 * caller's arrays of ndgpu_ovl_index_create).  opt->step must be 1, opt->mode not 3, k <= 28 (the compiled reference aborts on
 * ava-hifi -c);
 * with q == q2 and e == e2 the reference takes ksw_extz2_sse, which equals the two-piece kernel with equal pieces under the flags this path passes).
 * Every alignment runs on the device (one wavefront per problem, csrc/ksw2_kernels.hip); the joining of CIGARs, the z-drop
 * bookkeeping and the seed filters are host logic.  *recs is malloc'd (ndgpu_ovl_free).  Returns the record count, < 0 on error. */
int64_t ndgpu_ovl_map_cigar(ndgpu_ovl_index *idx, const ndgpu_ovl_opt *opt, const ndgpu_ovl_aln_opt *aopt, int32_t mid_occ,
                            uint32_t n_reads, const uint32_t *words, uint64_t n_words, const uint64_t *word_off, const uint32_t *lens,
                            const uint32_t *ids, const uint32_t *t_words, const uint64_t *t_word_off, const uint32_t *t_lens,
                            const uint32_t *t_ids, ndgpu_ovl_rec **recs, ndgpu_ovl_cigar_stats *stats);

void ndgpu_ovl_get_stats(const ndgpu_ovl_index *idx, ndgpu_ovl_stats *st);
void ndgpu_ovl_reset_stats(ndgpu_ovl_index *idx);

#pragma GCC visibility pop
#ifdef __cplusplus
}
#endif
#endif
