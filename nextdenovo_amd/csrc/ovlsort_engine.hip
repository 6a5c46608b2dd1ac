// ovlsort_engine.hip -- host orchestration + C ABI of the overlap sort / filter stage (util/ovl_sort.c path).
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <hip/hip_runtime.h>

#include "../../include/ndgpu_overlap.h"
#include "ovl_device.h"
#include "ovl_host.h"
#include "ovl_recset.h"

namespace ndovl {

void launch_expand_flags(const OvlRec *raw, uint64_t n, const uint32_t *seed_len, uint32_t n_ids, uint32_t *hq, uint32_t *ht, uint32_t *mq,
                         uint32_t *mt, hipStream_t s);
void launch_expand_count(uint64_t n, const uint32_t *file_of, const uint64_t *file_start, const uint32_t *hq, const uint32_t *ht,
                         const uint64_t *mqs, const uint64_t *mts, uint32_t *sel, hipStream_t s);
void launch_sel_count(const uint32_t *sel, uint64_t n, uint32_t *cnt, hipStream_t s);
void launch_expand_count_piece(uint64_t n, const uint32_t *hq, const uint32_t *ht, const uint64_t *mqs, const uint64_t *mts, uint64_t carry_q,
                               uint64_t carry_t, uint32_t *sel, hipStream_t s);
void launch_cand_hist(const OvlRec *raw, const uint32_t *sel, uint64_t n, uint32_t *hist, hipStream_t s);
void launch_range_sel(const OvlRec *raw, const uint8_t *sel, uint64_t n, uint32_t lo, uint32_t hi, uint32_t *out, hipStream_t s);
void launch_narrow_u32_u8(const uint32_t *in, uint64_t n, uint8_t *out, hipStream_t s);
void launch_expand_write(const OvlRec *raw, uint64_t n, const uint32_t *sel, const uint64_t *pos, OvlRec *cand, uint32_t *k_span,
                         uint32_t *k_match, uint32_t *k_seed, hipStream_t s);
void launch_iota(uint32_t *a, uint64_t n, hipStream_t s);
void launch_gather_u32(const uint32_t *src, const uint32_t *idx, uint64_t n, uint32_t *dst, hipStream_t s);
void launch_seed_flag(const OvlRec *cand, const uint32_t *perm, uint64_t n, uint32_t *flag, hipStream_t s);
void launch_seed_start(const uint32_t *flag, const uint64_t *rank, uint64_t n, uint64_t *start, hipStream_t s);
void sort_pairs_u32(void *tmp, size_t &tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                   hipStream_t s);
void launch_seed_filter(const OvlRec *cand, const uint32_t *perm, const uint64_t *seed_start, uint32_t n_seeds, uint64_t n_cand,
                        const uint32_t *seed_len, int max_bin_cov, int flank, int min_seed_len, uint32_t max_bins, uint32_t *kept, OvlRec *out,
                        uint32_t *n_out, uint32_t *bl_id, uint8_t *bl_kind, bool hq, hipStream_t s);
void launch_compact_seed_recs(const uint64_t *seed_start, uint32_t n_seeds, const OvlRec *out, const uint32_t *n_out, const uint64_t *off,
                              OvlRec *dense, hipStream_t s);
// K16, the pile admission (csrc/ovlsort_kernels.hip)
void launch_group_flag(const OvlRec *recs, uint64_t n, uint32_t *flag, hipStream_t s);
void launch_skip_bits(const uint32_t *ids, const uint8_t *kind, uint64_t n, uint32_t n_ids, uint32_t *bits, hipStream_t s);
uint32_t admit_lds_slots();
void launch_admit_plan(const uint64_t *off, uint32_t n_groups, uint32_t lds_slots, uint32_t *slots, uint32_t *counters, hipStream_t s);
void launch_admit_count(const OvlRec *recs, const uint64_t *off, uint32_t n_groups, const uint32_t *skip_bits, uint32_t n_ids,
                        uint32_t min_len_seed, uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, uint32_t lds_slots,
                        const uint32_t *wide_slots, const uint64_t *tab_off, uint64_t *scratch, uint8_t *adm, uint32_t *n_adm, uint32_t *kept,
                        uint32_t *counters, hipStream_t s);
void launch_admit_emit(const OvlRec *recs, const uint64_t *off, uint32_t n_groups, const uint8_t *adm, const uint32_t *n_adm,
                       const uint32_t *kept, const uint64_t *rec_off, const uint64_t *pile_idx, uint32_t *recs8, uint64_t *pile_off,
                       uint32_t *seeds, hipStream_t s);

// K17, the `.ovl` codec (csrc/ovlsort_kernels.hip)
uint32_t codec_tile_bytes();
void launch_codec_count(const uint8_t *img, const uint64_t *start, const uint64_t *bytes, const uint64_t *tile0, const uint32_t *tile_file,
                        uint64_t n_tiles, uint32_t *tile_cnt, hipStream_t s);
void launch_codec_file_plan(const uint64_t *tile0, const uint64_t *tile_first, uint32_t n_files, uint64_t *n_rec, hipStream_t s);
void launch_codec_emit(const uint8_t *img, const uint64_t *start, const uint64_t *bytes, const uint64_t *tile0, const uint32_t *tile_file,
                       uint64_t n_tiles, const uint64_t *tile_first, const uint64_t *n_rec, const uint64_t *rec_base, OvlRec *recs,
                       uint64_t *consumed, hipStream_t s);
void launch_codec_delta(const OvlRec *recs, uint64_t n, uint32_t *dq, uint32_t *dt, hipStream_t s);
void launch_codec_records(OvlRec *recs, uint64_t n, const uint32_t *dq, const uint32_t *dt, const uint64_t *sq, const uint64_t *st,
                          const uint64_t *rec_base, uint32_t n_files, hipStream_t s);
void launch_codec_size(const OvlRec *recs, uint64_t n, uint32_t prev_q, uint32_t prev_t, uint32_t *len, hipStream_t s);
void launch_codec_write(const OvlRec *recs, uint64_t n, uint32_t prev_q, uint32_t prev_t, const uint64_t *off, uint8_t *out, hipStream_t s);

// K18, the stable split of a record set, and the file of every record of a sort's input (csrc/ovlsort_kernels.hip)
uint32_t split_tile_records();
uint32_t split_max_files();
void launch_split_count(const OvlRec *recs, uint64_t n, const uint32_t *file_of, uint32_t n_ids, uint32_t n_files, uint64_t n_tiles, uint32_t *cnt,
                        uint32_t *bad_cnt, hipStream_t s);
void launch_split_cuts(const uint64_t *first, uint64_t n_tiles, uint32_t n_files, uint64_t *cuts, hipStream_t s);
void launch_split_scatter(const OvlRec *recs, uint64_t n, const uint32_t *file_of, uint32_t n_ids, uint32_t n_files, uint64_t n_tiles,
                          const uint64_t *first, OvlRec *out, hipStream_t s);
void launch_file_fill(const uint64_t *fstart, uint32_t n_files, uint64_t n, uint32_t *file_of, hipStream_t s);

struct SortRun {
	hipStream_t st = nullptr;
	Scratch tmp{256};
	void exscan(const uint32_t *in, uint64_t *out, size_t n)
	{
		tmp.run([&](void *t, size_t &tb) { exscan_u32_to_u64(t, tb, in, out, n, st); });
	}
	// stable LSD pass: reorder perm by key[perm]
	void pass(const uint32_t *key, uint32_t *perm, uint32_t *perm2, uint32_t *k1, uint32_t *k2, size_t n)
	{
		launch_gather_u32(key, perm, n, k1, st);
		tmp.run([&](void *t, size_t &tb) { sort_pairs_u32(t, tb, k1, k2, perm, perm2, n, st); });
		HIP_OK(hipMemcpyAsync(perm, perm2, n * 4, hipMemcpyDeviceToDevice, st));
	}
};

} // namespace ndovl

using namespace ndovl;

// the records of a call, in the malloc'd block the caller gets (grown by realloc when a call sorts in seed ranges): the download
// goes straight into it -- through a std::vector the records were zero-filled, downloaded and copied once more, 5 ms per 18 MB
struct RecOut {
	OvlRec *p = nullptr;
	size_t n = 0, cap = 0;
	~RecOut() { free(p); }
	RecOut() = default;
	RecOut(const RecOut &) = delete;
	RecOut &operator=(const RecOut &) = delete;
	size_t size() const { return n; }
	OvlRec *grow(size_t more) {   // room for `more` records at the end; returns where they go
		if (n + more + 1 > cap) {
			const size_t want = std::max(n + more + 1, cap + cap / 2);
			OvlRec *q = (OvlRec*)realloc(p, want * sizeof(OvlRec));
			if (!q) throw std::runtime_error("malloc");
			p = q, cap = want;
		}
		OvlRec *at = p + n;
		n += more;
		return at;
	}
	OvlRec *release() { OvlRec *q = p ? p : (OvlRec*)malloc(sizeof(OvlRec)); p = nullptr, n = cap = 0; return q; }
};

struct SortOut {
	RecOut recs;
	std::vector<uint32_t> bl_id;
	std::vector<uint8_t> bl_kind;
	uint64_t seeds = 0, n_recs = 0;   // n_recs: sorted records, downloaded or not
};

// The admission tail of a call (K16): the thresholds, the skip set as a bitmap on the device, and what was admitted so far -- the
// seed ranges of the out-of-core sort are independent, their piles are appended in order.  A row of recs8 is as wide as a record,
// so the rows grow in a RecOut too.
struct Admission {
	uint32_t n_ids = 0, min_len_seed = 0, min_len_aln = 0, max_cov_aln = 0, min_cov_seed = 0, lds_slots = 0;
	bool use_bl = false, want_sorted = false, declined = false;
	DevBuf<uint32_t> skip_bits;
	RecOut rows;
	std::vector<uint64_t> pile_off{0};
	std::vector<uint32_t> seeds;
	ndgpu_ovl_admit_stats st{};

	Admission(uint32_t ids, uint32_t mls, uint32_t mla, uint32_t mca, uint32_t mcs)
		: n_ids(ids), min_len_seed(mls), min_len_aln(mla), max_cov_aln(mca), min_cov_seed(mcs) {}
	void begin(const uint32_t *skip_ids, int64_t n_skip, hipStream_t s)
	{
		// the LDS table's capacity, a power of two; NDGPU_ADMIT_TABLE=<slots> forces a smaller one (groups of more than half of it
		// take the table in global memory: the wide path on small inputs)
		lds_slots = admit_lds_slots();
		if (const char *e = getenv("NDGPU_ADMIT_TABLE")) {
			const uint64_t v = strtoull(e, nullptr, 10);
			uint32_t p = 2;
			while ((uint64_t)p * 2 <= v && p * 2 <= lds_slots) p *= 2;
			lds_slots = p;
		}
		skip_bits.alloc((size_t)(n_ids >> 5) + 2);
		skip_bits.zero(s);
		if (n_skip > 0) {
			DevBuf<uint32_t> ids_d((size_t)n_skip);
			ids_d.upload(skip_ids, (size_t)n_skip, s);
			launch_skip_bits(ids_d.p, nullptr, (uint64_t)n_skip, n_ids, skip_bits.p, s);
			HIP_OK(hipStreamSynchronize(s));   // (ids_d goes back to the pool)
		}
	}
	void hand_out(uint32_t **recs8, uint64_t **poff, uint32_t **sd, int64_t *n_piles)
	{
		*poff = malloc_copy<uint64_t>(pile_off);
		*sd = malloc_copy<uint32_t>(seeds);
		*n_piles = (int64_t)seeds.size();
		*recs8 = (uint32_t*)rows.release();
		if (!*recs8) throw std::runtime_error("malloc");
	}
};

// ---- K17, the `.ovl` codec on the device: the host side ----
// the byte images of a call's files, as the caller holds them
struct ImageSet {
	const uint8_t *const *bufs;
	const uint64_t *n_bytes;
	int32_t n_files;
	uint64_t total() const { uint64_t t = 0; for (int f = 0; f < n_files; ++f) t += n_bytes[f]; return t; }
};

// the host loop over every file (the cross-check, and the decode of a call that sorts out of core): records in file order
static void decode_on_host(const ImageSet &I, RecOut &out, std::vector<int64_t> &n_per_file, uint64_t *consumed)
{
	n_per_file.assign((size_t)I.n_files, 0);
	for (int f = 0; f < I.n_files; ++f) {
		const uint64_t cap = I.n_bytes[f] / 8;   // a record is 8 bytes at least
		OvlRec *const at = out.grow(cap);
		uint32_t prev[2] = {0, 0};
		uint64_t used = 0;
		const int64_t n = cap ? ndgpu_ovl_decode(I.bufs[f], I.n_bytes[f], prev, (uint32_t*)at, (int64_t)cap, &used) : 0;
		for (int64_t i = 0; i < n; ++i) {   // decode_ovl's field order -> the record's
			const uint32_t *o = (const uint32_t*)(at + i);
			const OvlRec r = {o[1], o[0], o[2], o[3], o[4], o[5], o[6], o[7]};
			at[i] = r;
		}
		out.n -= cap - (uint64_t)n;
		n_per_file[(size_t)f] = n;
		if (consumed) consumed[f] = used;
	}
}

// Decode in two steps, so that a caller can size its buffers (or turn to another path) between them: count() uploads the images
// and finds every file's whole records, emit() writes them to device memory the caller names.
struct DecodeRun {
	DevBuf<uint8_t> img;
	DevBuf<uint64_t> start, bytes, tile0, tile_first, n_rec_d;
	DevBuf<uint32_t> tile_file;
	uint64_t n_tiles = 0, total = 0;
	uint32_t n_files = 0;
	std::vector<uint64_t> n_rec, base;   // per file: whole records, first record (n_files + 1 entries)

	void count(SortRun &R, const ImageSet &I)
	{
		const uint64_t tile = codec_tile_bytes();
		n_files = (uint32_t)I.n_files;
		std::vector<uint64_t> h_start(n_files + 1), h_bytes(n_files + 1, 0), h_tile0(n_files + 1);
		for (uint32_t f = 0; f < n_files; ++f) {
			h_start[f] = n_tiles * tile, h_tile0[f] = n_tiles, h_bytes[f] = I.n_bytes[f];
			n_tiles += (I.n_bytes[f] + tile - 1) / tile;
		}
		h_start[n_files] = n_tiles * tile, h_tile0[n_files] = n_tiles;
		if (n_tiles >= 0x7fffffffull) throw std::runtime_error("too many bytes for one decode call");
		std::vector<uint32_t> h_tile_file(n_tiles);
		for (uint32_t f = 0; f < n_files; ++f) std::fill(h_tile_file.begin() + h_tile0[f], h_tile_file.begin() + h_tile0[f + 1], f);
		n_rec.assign(n_files, 0), base.assign((size_t)n_files + 1, 0);
		if (n_tiles == 0) return;
		img.alloc(n_tiles * tile);
		for (uint32_t f = 0; f < n_files; ++f)
			if (h_bytes[f]) HIP_OK(hipMemcpyAsync(img.p + h_start[f], I.bufs[f], h_bytes[f], hipMemcpyHostToDevice, R.st));
		start.alloc(n_files + 1), bytes.alloc(n_files + 1), tile0.alloc(n_files + 1), tile_file.alloc(n_tiles);
		start.upload(h_start.data(), n_files + 1, R.st), bytes.upload(h_bytes.data(), n_files + 1, R.st);
		tile0.upload(h_tile0.data(), n_files + 1, R.st), tile_file.upload(h_tile_file.data(), n_tiles, R.st);
		DevBuf<uint32_t> tile_cnt(n_tiles + 1);
		tile_cnt.zero(R.st);
		tile_first.alloc(n_tiles + 1), n_rec_d.alloc(n_files);
		launch_codec_count(img.p, start.p, bytes.p, tile0.p, tile_file.p, n_tiles, tile_cnt.p, R.st);
		R.exscan(tile_cnt.p, tile_first.p, n_tiles + 1);
		launch_codec_file_plan(tile0.p, tile_first.p, n_files, n_rec_d.p, R.st);
		n_rec_d.download(n_rec.data(), n_files, R.st);
		HIP_OK(hipStreamSynchronize(R.st));   // (the host vectors of the uploads above live until here)
		HIP_OK(hipGetLastError());
		for (uint32_t f = 0; f < n_files; ++f) base[f + 1] = base[f] + n_rec[f];
		total = base[n_files];
	}
	// the records to out[0 .. total); consumed (n_files entries) may be null
	void emit(SortRun &R, OvlRec *out, uint64_t *consumed)
	{
		if (consumed) std::fill(consumed, consumed + n_files, 0);
		if (total == 0) return;
		DevBuf<uint64_t> rec_base((size_t)n_files + 1), used(n_files), sq(total), st(total);
		DevBuf<uint32_t> dq(total), dt(total);
		rec_base.upload(base.data(), (size_t)n_files + 1, R.st);
		used.zero(R.st);
		launch_codec_emit(img.p, start.p, bytes.p, tile0.p, tile_file.p, n_tiles, tile_first.p, n_rec_d.p, rec_base.p, out, used.p, R.st);
		launch_codec_delta(out, total, dq.p, dt.p, R.st);
		R.exscan(dq.p, sq.p, total);
		R.exscan(dt.p, st.p, total);
		launch_codec_records(out, total, dq.p, dt.p, sq.p, st.p, rec_base.p, n_files, R.st);
		if (consumed) used.download(consumed, n_files, R.st);
		HIP_OK(hipStreamSynchronize(R.st));   // (the scratch buffers of this call go back to the pool)
		HIP_OK(hipGetLastError());
	}
	void release() { img.release(), tile_first.release(), tile_file.release(); }
};

// bytes handed to the caller in one malloc'd block that grows as the seed ranges of a call are encoded
struct ByteOut {
	uint8_t *p = nullptr;
	size_t n = 0, cap = 0;
	~ByteOut() { free(p); }
	ByteOut() = default;
	ByteOut(const ByteOut &) = delete;
	ByteOut &operator=(const ByteOut &) = delete;
	uint8_t *grow(size_t more)
	{
		if (n + more + 1 > cap) {
			const size_t want = std::max(n + more + 1, cap + cap / 2);
			uint8_t *q = (uint8_t*)realloc(p, want);
			if (!q) throw std::runtime_error("malloc");
			p = q, cap = want;
		}
		uint8_t *at = p + n;
		n += more;
		return at;
	}
	uint8_t *release()   // at exact size (one byte when there is none), never null
	{
		uint8_t *q = (uint8_t*)realloc(p, n ? n : 1);
		if (!q) throw std::runtime_error("malloc");
		p = nullptr, n = cap = 0;
		return q;
	}
};

// The encode tail of a call: device records in, their bytes appended to the image, `prev` carried from one append to the next
// (the seed ranges of the out-of-core sort are one file).
struct EncodeTail {
	uint32_t prev[2] = {0, 0};
	ByteOut image;
	ndgpu_ovl_codec_stats st{};
	void append(SortRun &R, const OvlRec *recs, uint64_t n)
	{
		if (n == 0) return;
		EvTimer tm(R.st);
		tm.start();
		DevBuf<uint32_t> len(n + 1);
		DevBuf<uint64_t> off(n + 1);
		HIP_OK(hipMemsetAsync(len.p + n, 0, sizeof(uint32_t), R.st));
		launch_codec_size(recs, n, prev[0], prev[1], len.p, R.st);
		R.exscan(len.p, off.p, n + 1);
		uint64_t nb = 0;
		OvlRec last;
		off.download(&nb, 1, R.st, n);
		HIP_OK(hipMemcpyAsync(&last, recs + (n - 1), sizeof(OvlRec), hipMemcpyDeviceToHost, R.st));
		HIP_OK(hipStreamSynchronize(R.st));
		HIP_OK(hipGetLastError());
		if (nb < 8 * n || nb > 40 * n) throw std::runtime_error("encoded size out of range");
		DevBuf<uint8_t> out(nb + 4);
		launch_codec_write(recs, n, prev[0], prev[1], off.p, out.p, R.st);
		st.encode_ms += tm.stop();
		uint8_t *const dst = image.grow(nb);
		out.download(dst, nb, R.st);
		HIP_OK(hipStreamSynchronize(R.st));
		HIP_OK(hipGetLastError());
		prev[0] = last.qname, prev[1] = last.tname;
		st.bytes_out += nb, st.bytes_downloaded += nb;
	}
};

// K16 over `n` dense sorted records in `n_groups` groups (group g = dense[off[g] .. off[g + 1]); off has n_groups + 1 entries):
// count, two scans, emit; the piles are appended to A.  An irregular group turns the call over to the host routine (A.declined).
static void admit_tail(SortRun &R, const OvlRec *dense, const uint64_t *off, uint64_t n_groups, uint64_t n, Admission &A)
{
	A.st.sorted_records += n, A.st.groups += n_groups;
	if (A.declined || n_groups == 0 || n == 0) return;
	if (n >= (1ull << 30) || n_groups >= 0x7fffffffull) throw std::runtime_error("too many records for one admission call");
	const uint32_t G = (uint32_t)n_groups;
	EvTimer tm(R.st);
	tm.start();
	DevBuf<uint8_t> adm(n + 1);
	DevBuf<uint32_t> n_adm(G + 1), kept(G + 1), slots(G + 1), counters(4);
	DevBuf<uint64_t> rec_off(G + 1), pile_idx(G + 1), tab_off(G + 1);
	// a wide group of c records takes pow2ceil(2 c) < 4 c slots, and no group is wide when all records together are not
	DevBuf<uint64_t> scratch(2 * n > A.lds_slots ? 4 * n + 1 : 1);
	adm.zero(R.st), n_adm.zero(R.st), kept.zero(R.st), slots.zero(R.st), counters.zero(R.st);
	launch_admit_plan(off, G, A.lds_slots, slots.p, counters.p, R.st);
	R.exscan(slots.p, tab_off.p, (size_t)G + 1);
	launch_admit_count(dense, off, G, A.skip_bits.p, A.n_ids, A.min_len_seed, A.min_len_aln, A.max_cov_aln, A.min_cov_seed, A.lds_slots, slots.p,
	                   tab_off.p, scratch.p, adm.p, n_adm.p, kept.p, counters.p, R.st);
	R.exscan(n_adm.p, rec_off.p, (size_t)G + 1);
	R.exscan(kept.p, pile_idx.p, (size_t)G + 1);
	uint64_t n_rows = 0, n_piles = 0;
	uint32_t h_counters[4] = {0, 0, 0, 0};
	rec_off.download(&n_rows, 1, R.st, G);
	pile_idx.download(&n_piles, 1, R.st, G);
	counters.download(h_counters, 4, R.st);
	HIP_OK(hipStreamSynchronize(R.st));
	HIP_OK(hipGetLastError());
	A.st.groups_declined += h_counters[0], A.st.groups_wide += h_counters[1];
	A.st.bytes_downloaded += 32;
	if (h_counters[0]) {
		A.declined = true;
		A.st.k16_ms += tm.stop();
		return;
	}
	if (n_rows > n || n_piles > n_groups) throw std::runtime_error("admission counts out of range");
	DevBuf<uint32_t> r8(n_rows * 8 + 8), sd(n_piles + 1);
	DevBuf<uint64_t> poff(n_piles + 1);
	launch_admit_emit(dense, off, G, adm.p, n_adm.p, kept.p, rec_off.p, pile_idx.p, r8.p, poff.p, sd.p, R.st);
	const uint64_t row_base = A.pile_off.back();
	const size_t pile_base = A.seeds.size();
	A.pile_off.pop_back();
	A.pile_off.resize(pile_base + n_piles + 1);
	A.seeds.resize(pile_base + n_piles);
	uint32_t *const dst = (uint32_t*)A.rows.grow(n_rows);
	r8.download(dst, n_rows * 8, R.st);
	poff.download(A.pile_off.data() + pile_base, n_piles, R.st);
	sd.download(A.seeds.data() + pile_base, n_piles, R.st);
	A.st.k16_ms += tm.stop();   // (waits for the stream: the downloads above are in)
	HIP_OK(hipGetLastError());
	for (uint64_t p = 0; p < n_piles; ++p) A.pile_off[pile_base + p] += row_base;
	A.pile_off[pile_base + n_piles] = row_base + n_rows;
	A.st.admitted += n_rows, A.st.piles += n_piles;
	A.st.bytes_downloaded += n_rows * 32 + n_piles * 12;
}

// S2 + S3 over one set of candidates (all of a call, or those of one seed range): the sorted, filtered records and the `.bl`
// verdicts are appended to `o`
static void sort_and_filter(SortRun &R, const OvlRec *cand_p, const uint32_t *k_span_p, const uint32_t *k_match_p, const uint32_t *k_seed_p,
                            uint64_t nc, const uint32_t *d_seed_p, const uint32_t *seed_len, uint32_t n_ids, int32_t min_seed_len,
                            int32_t max_bin_cov, int32_t max_flank_len, bool hq_mode, SortOut &o, Admission *A = nullptr,
                            EncodeTail *E = nullptr)
{
	DevBuf<uint32_t> perm(nc), perm2(nc), k1(nc), k2(nc);
	// S2: (seed asc, match desc, span asc), stable
	launch_iota(perm.p, nc, R.st);
	R.pass(k_span_p, perm.p, perm2.p, k1.p, k2.p, nc);
	R.pass(k_match_p, perm.p, perm2.p, k1.p, k2.p, nc);
	R.pass(k_seed_p, perm.p, perm2.p, k1.p, k2.p, nc);

	// seeds
	DevBuf<uint32_t> flag(nc + 1);
	DevBuf<uint64_t> rank(nc + 1);
	flag.zero(R.st);
	launch_seed_flag(cand_p, perm.p, nc, flag.p, R.st);
	R.exscan(flag.p, rank.p, nc + 1);
	uint64_t n_seeds = 0;
	rank.download(&n_seeds, 1, R.st, nc);
	HIP_OK(hipStreamSynchronize(R.st));
	DevBuf<uint64_t> sstart(n_seeds + 1);
	launch_seed_start(flag.p, rank.p, nc, sstart.p, R.st);

	// S3
	uint32_t max_len = 0;
	for (uint32_t i = 0; i < n_ids; ++i) max_len = std::max(max_len, seed_len[i]);
	const uint32_t max_bins = (max_len >> 6) + 2;
	DevBuf<uint32_t> kept(nc + n_seeds + 1), n_out(n_seeds + 1), d_bl_id(n_seeds + 1);
	DevBuf<uint8_t> d_bl_kind(n_seeds + 1);
	DevBuf<OvlRec> outrec(nc + n_seeds + 1);
	n_out.zero(R.st);
	launch_seed_filter(cand_p, perm.p, sstart.p, (uint32_t)n_seeds, nc, d_seed_p, max_bin_cov, max_flank_len, min_seed_len, max_bins, kept.p,
	                   outrec.p, n_out.p, d_bl_id.p, d_bl_kind.p, hq_mode, R.st);
	DevBuf<uint64_t> off(n_seeds + 1);
	R.exscan(n_out.p, off.p, n_seeds + 1);
	uint64_t total = 0;
	off.download(&total, 1, R.st, n_seeds);
	HIP_OK(hipStreamSynchronize(R.st));
	HIP_OK(hipGetLastError());
	DevBuf<OvlRec> dense(total + 1);
	launch_compact_seed_recs(sstart.p, (uint32_t)n_seeds, outrec.p, n_out.p, off.p, dense.p, R.st);
	std::vector<uint32_t> h_id(n_seeds);
	std::vector<uint8_t> h_kind(n_seeds);
	if (E) {   // the sorted records leave as their `.ovl` bytes (K17): encoded where they lie
		E->append(R, dense.p, total);
	} else if (!A || A->want_sorted) {
		OvlRec *const dst = o.recs.grow(total);
		dense.download(dst, total, R.st);
	}
	o.n_recs += total;
	d_bl_id.download(h_id.data(), n_seeds, R.st);
	d_bl_kind.download(h_kind.data(), n_seeds, R.st);
	HIP_OK(hipStreamSynchronize(R.st));
	HIP_OK(hipGetLastError());
	for (uint64_t i = 0; i < n_seeds; ++i)
		if (h_kind[i]) o.bl_id.push_back(h_id[i]), o.bl_kind.push_back(h_kind[i]);
	o.seeds += n_seeds;
	if (A) {   // the admission on dense / off / the verdicts while they are on the device
		A->st.bytes_downloaded += n_seeds * 5 + (A->want_sorted ? total * sizeof(OvlRec) : 0);
		if (A->use_bl) launch_skip_bits(d_bl_id.p, d_bl_kind.p, n_seeds, A->n_ids, A->skip_bits.p, R.st);
		admit_tail(R, dense.p, off.p, n_seeds, total, *A);
	}
}

static void hand_out(SortOut &so, ndgpu_ovl_rec **out, uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl)
{
	static_assert(sizeof(OvlRec) == sizeof(ndgpu_ovl_rec), "record layout");
	*bl_id = malloc_copy<uint32_t>(so.bl_id);
	*bl_kind = malloc_copy<uint8_t>(so.bl_kind);
	*out = (ndgpu_ovl_rec*)so.recs.release();
	if (!*out) throw std::runtime_error("malloc");
	*n_bl = (int64_t)so.bl_id.size();
}

// The sort when the candidates of a seed file do not fit the device at once (`ovl_sort -m` with less memory than data: the
// reference spills sorted runs to temporary files and merges them, util/ovl_sort.c:1079-1110; the result does not depend on -m).
// Here the raw records stay in host memory (the caller's arrays) and pass the device twice, in pieces:
//   pass A  per piece of a file: which sides of which records become candidates (the "5 misses then stop" rule is per file, so
//           a piece carries the miss counts of the file's earlier pieces), one byte per record kept on the host, and a histogram of
//           candidates per seed;
//   the seeds are cut into consecutive id ranges whose candidates fit;
//   pass B  per range: every piece again, only the sides whose seed lies in the range are expanded; S2 + S3 on them.
// A seed's records depend on its own candidates only and the output is in seed order, so the ranges' outputs, one after the other,
// are the output of the whole sort; equal (seed, match, span) keys keep input order in either form.
static void sort_out_of_core(SortRun &R, const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                             uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, bool hq_mode, uint64_t piece_cap,
                             uint64_t range_cap, SortOut &so, uint64_t *nc_total, uint64_t *n_ranges, Admission *A, EncodeTail *E)
{
	DevBuf<uint32_t> d_seed(n_ids + 1), hist(n_ids + 1);
	d_seed.upload(seed_len, n_ids, R.st);
	hist.zero(R.st);
	std::vector<std::vector<uint8_t>> sel_of((size_t)n_files);
	DevBuf<OvlRec> raw(piece_cap);
	DevBuf<uint32_t> hq(piece_cap + 1), ht(piece_cap + 1), mq(piece_cap + 1), mt(piece_cap + 1), sel(piece_cap + 1), cnt(piece_cap + 1);
	DevBuf<uint64_t> mqs(piece_cap + 1), mts(piece_cap + 1), pos(piece_cap + 1);
	DevBuf<uint8_t> sel8(piece_cap + 1);
	for (int f = 0; f < n_files; ++f) {  // pass A
		const uint64_t nf = (uint64_t)n_per_file[f];
		sel_of[(size_t)f].resize(nf);
		uint64_t carry_q = 0, carry_t = 0;
		for (uint64_t a = 0; a < nf; a += piece_cap) {
			const uint64_t m = std::min<uint64_t>(piece_cap, nf - a);
			raw.upload((const OvlRec*)files[f] + a, m, R.st);
			mq.zero(m + 1, R.st);
			mt.zero(m + 1, R.st);
			launch_expand_flags(raw.p, m, d_seed.p, n_ids, hq.p, ht.p, mq.p, mt.p, R.st);
			R.exscan(mq.p, mqs.p, m + 1);
			R.exscan(mt.p, mts.p, m + 1);
			launch_expand_count_piece(m, hq.p, ht.p, mqs.p, mts.p, carry_q, carry_t, sel.p, R.st);
			launch_cand_hist(raw.p, sel.p, m, hist.p, R.st);
			launch_narrow_u32_u8(sel.p, m, sel8.p, R.st);
			uint64_t dq = 0, dt = 0;
			sel8.download(sel_of[(size_t)f].data() + a, m, R.st);
			mqs.download(&dq, 1, R.st, m);
			mts.download(&dt, 1, R.st, m);
			HIP_OK(hipStreamSynchronize(R.st));
			carry_q += dq, carry_t += dt;
		}
	}
	std::vector<uint32_t> h_hist((size_t)n_ids + 1);
	hist.download(h_hist.data(), (size_t)n_ids + 1, R.st);
	HIP_OK(hipStreamSynchronize(R.st));
	*nc_total = 0, *n_ranges = 0;
	for (uint32_t lo = 0; lo < n_ids;) {  // pass B, range by range
		uint64_t nc = h_hist[lo];
		uint32_t hi = lo + 1;
		while (hi < n_ids && nc + h_hist[hi] <= range_cap) nc += h_hist[hi++];
		if (nc == 0) { lo = hi; continue; }
		if (nc >= 0x7fffffffull) throw std::runtime_error("one seed has more than 2^31 candidates");
		DevBuf<OvlRec> cand(nc);
		DevBuf<uint32_t> k_span(nc), k_match(nc), k_seed(nc);
		uint64_t base = 0;
		for (int f = 0; f < n_files; ++f) {
			const uint64_t nf = (uint64_t)n_per_file[f];
			for (uint64_t a = 0; a < nf; a += piece_cap) {
				const uint64_t m = std::min<uint64_t>(piece_cap, nf - a);
				raw.upload((const OvlRec*)files[f] + a, m, R.st);
				sel8.upload(sel_of[(size_t)f].data() + a, m, R.st);
				cnt.zero(m + 1, R.st);
				launch_range_sel(raw.p, sel8.p, m, lo, hi, sel.p, R.st);
				launch_sel_count(sel.p, m, cnt.p, R.st);
				R.exscan(cnt.p, pos.p, m + 1);
				uint64_t got = 0;
				pos.download(&got, 1, R.st, m);
				HIP_OK(hipStreamSynchronize(R.st));
				if (base + got > nc) throw std::runtime_error("candidate count changed between the passes");
				launch_expand_write(raw.p, m, sel.p, pos.p, cand.p + base, k_span.p + base, k_match.p + base, k_seed.p + base, R.st);
				HIP_OK(hipStreamSynchronize(R.st));  // (raw / sel are reused by the next piece)
				base += got;
			}
		}
		if (base != nc) throw std::runtime_error("candidate count changed between the passes");
		sort_and_filter(R, cand.p, k_span.p, k_match.p, k_seed.p, nc, d_seed.p, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, hq_mode, so, A, E);
		*nc_total += nc, ++*n_ranges;
		lo = hi;
	}
}

static int64_t sort_impl(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                         uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, ndgpu_ovl_rec **out,
                         uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats, bool hq_mode, Admission *A = nullptr,
                         const uint32_t *skip_ids = nullptr, int64_t n_skip = 0, const ImageSet *images = nullptr, EncodeTail *E = nullptr,
                         const ndgpu_ovl_recset *const *sets = nullptr)
{
	*out = nullptr, *bl_id = nullptr, *bl_kind = nullptr, *n_bl = 0;
	if (stats) memset(stats, 0, sizeof(*stats));
	const bool prof = getenv("NDGPU_PROF") != nullptr;
	const auto tp0 = std::chrono::steady_clock::now();
	auto since = [&] { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tp0).count(); };
	try {
		if (select_device(true) < 0) return -1;
		SortRun R;
		HIP_OK(ndovl::create_stage_stream(&R.st));
		const StreamGuard guard{R.st};
		EvTimer tm(R.st);
		tm.start();
		const double t_setup = since();

		// in one piece when the device holds the raw records, their flags and up to two candidates per record (~360 bytes per record
		// with the sort's scratch); otherwise -- or when told to -- in seed ranges (sort_out_of_core)
		uint64_t piece_cap = 0, range_cap = 0;
		if (const char *e = getenv("NDGPU_OVLSORT_PIECE_RECORDS")) piece_cap = strtoull(e, nullptr, 10);
		if (const char *e = getenv("NDGPU_OVLSORT_RANGE_CANDIDATES")) range_cap = strtoull(e, nullptr, 10);
		uint64_t avail = 0;
		auto fits = [&](uint64_t recs) { return !(piece_cap || range_cap || recs * 360ull > avail || 2 * recs >= 0x7fffffffull); };
		auto look_at_memory = [&] {
			size_t mem_free = 0, mem_total = 0;
			HIP_OK(hipMemGetInfo(&mem_free, &mem_total));
			avail = (uint64_t)mem_free + (uint64_t)pool_cached_bytes();
			// NDGPU_OVLSORT_AVAIL_BYTES=<bytes>: the figure to decide on instead (a test hook, like the two knobs above)
			if (const char *e = getenv("NDGPU_OVLSORT_AVAIL_BYTES")) avail = strtoull(e, nullptr, 10);
		};

		// the files as `.ovl` images (K17): counted on the device, and decoded straight into `raw` below when the sort is in one
		// piece; a sort in seed ranges reads its files from host memory, piece by piece and twice, so it gets them decoded on the host.
		// The form of the sort is decided HERE for a call with images, once, on the memory seen before the images went up: deciding
		// again below, with the images resident, could turn an in-core verdict around when no host records exist.
		DecodeRun D;
		RecOut host_recs;
		std::vector<const ndgpu_ovl_rec*> host_files;
		std::vector<int64_t> host_counts;
		bool raw_on_device = false;
		if (images) {
			n_files = images->n_files;
			const uint64_t img_bytes = images->total();
			look_at_memory();
			bool on_device = img_bytes > 0 && fits(img_bytes / 40);   // (a record is 40 bytes at most)
			if (on_device) {
				EvTimer dtm(R.st);
				dtm.start();
				D.count(R, *images);
				if (E) E->st.decode_ms += dtm.stop();
				on_device = fits(D.total);
			}
			uint64_t at = 0;
			if (on_device) {   // no host records: `files` stays null
				raw_on_device = true;
				host_counts.assign(D.n_rec.begin(), D.n_rec.end());
				at = D.total;
				if (E) E->st.bytes_uploaded += img_bytes;
			} else {
				D.release();
				decode_on_host(*images, host_recs, host_counts, nullptr);
				if (E && img_bytes) E->st.host_decodes += (uint64_t)n_files;
				for (int f = 0; f < n_files; ++f) host_files.push_back((const ndgpu_ovl_rec*)host_recs.p + at), at += (uint64_t)host_counts[(size_t)f];
				files = host_files.data();
			}
			n_per_file = host_counts.data();
			if (E) E->st.bytes_in += img_bytes, E->st.records += at;
		}

		// the files as record sets (ovl_recset.h): the form of the sort is decided HERE, once, as for images.  In one piece the sets
		// are copied into `raw` device to device below; a sort in seed ranges reads its files from host memory, piece by piece and
		// twice, so it gets them downloaded once into a block this call owns and goes on as a call with host records.
		bool from_sets = false;
		if (sets) {
			host_counts.assign((size_t)n_files, 0);
			uint64_t total = 0;
			for (int f = 0; f < n_files; ++f) host_counts[(size_t)f] = sets[f] ? (int64_t)sets[f]->n : 0, total += (uint64_t)host_counts[(size_t)f];
			n_per_file = host_counts.data();
			look_at_memory();
			from_sets = fits(total);
			if (!from_sets) {
				OvlRec *at = host_recs.grow(total);
				for (int f = 0; f < n_files; ++f) {
					const uint64_t m = (uint64_t)host_counts[(size_t)f];
					if (m) HIP_OK(hipMemcpyAsync(at, sets[f]->data(), m * sizeof(OvlRec), hipMemcpyDeviceToHost, R.st));
					host_files.push_back((const ndgpu_ovl_rec*)at), at += m;
				}
				HIP_OK(hipStreamSynchronize(R.st));
				files = host_files.data();
				g_recset.sets_downloaded += (uint64_t)n_files, g_recset.bytes_downloaded += total * sizeof(OvlRec);
			}
		}

		uint64_t n = 0;
		std::vector<uint64_t> h_fstart((size_t)n_files + 1);
		for (int f = 0; f < n_files; ++f) { h_fstart[f] = n; n += (uint64_t)n_per_file[f]; }
		h_fstart[n_files] = n;
		SortOut so;
		if (n == 0) { hand_out(so, out, bl_id, bl_kind, n_bl); return 0; }   // (nothing in: an empty result, the stats stay zero)
		if (A) A->begin(skip_ids, n_skip, R.st);
		if (!images && !sets) look_at_memory();
		const bool in_core = images ? raw_on_device : sets ? from_sets : fits(n);
		uint64_t nc = 0, n_ranges = 1;
		if (!in_core) {
			if (raw_on_device || !files) throw std::runtime_error("a sort in seed ranges needs its records in host memory");
			if (!piece_cap) piece_cap = std::max<uint64_t>(1u << 20, std::min<uint64_t>(n, avail / 8 / 96));
			if (!range_cap) range_cap = std::max<uint64_t>(1u << 20, std::min<uint64_t>(0x7ffffff0ull, avail / 2 / 180));
			sort_out_of_core(R, files, n_per_file, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, hq_mode, piece_cap, range_cap, so,
			                 &nc, &n_ranges, A, E);
		} else {
			std::vector<uint32_t> h_file_of(from_sets ? 0 : n);
			DevBuf<OvlRec> raw(n);
			for (int f = 0; f < n_files && from_sets; ++f)   // the sets' records: device to device on the sort's stream
				if (n_per_file[f])
					HIP_OK(hipMemcpyAsync(raw.p + h_fstart[f], sets[f]->data(), (size_t)n_per_file[f] * sizeof(OvlRec), hipMemcpyDeviceToDevice, R.st));
			if (from_sets) g_recset.bytes_d2d += n * sizeof(OvlRec);
			for (int f = 0; f < n_files && !from_sets; ++f) {
				std::fill(h_file_of.begin() + h_fstart[f], h_file_of.begin() + h_fstart[f + 1], (uint32_t)f);
				if (n_per_file[f] && !raw_on_device)
					HIP_OK(hipMemcpyAsync(raw.p + h_fstart[f], files[f], (size_t)n_per_file[f] * sizeof(OvlRec), hipMemcpyHostToDevice, R.st));
			}
			if (raw_on_device) {   // the records come out of the images the device already holds
				EvTimer dtm(R.st);
				dtm.start();
				D.emit(R, raw.p, nullptr);
				if (E) E->st.decode_ms += dtm.stop();
				D.release();
			}
			DevBuf<uint32_t> file_of(n), d_seed(n_ids + 1);
			DevBuf<uint64_t> fstart((size_t)n_files + 1);
			if (!from_sets) file_of.upload(h_file_of.data(), n, R.st);
			fstart.upload(h_fstart.data(), (size_t)n_files + 1, R.st);
			if (from_sets) launch_file_fill(fstart.p, (uint32_t)n_files, n, file_of.p, R.st);   // (no n-entry host vector, no upload of it)
			d_seed.upload(seed_len, n_ids, R.st);

			// S1: candidates
			DevBuf<uint32_t> hq(n + 1), ht(n + 1), mq(n + 1), mt(n + 1), sel(n + 1), cnt(n + 1);
			DevBuf<uint64_t> mqs(n + 1), mts(n + 1), pos(n + 1);
			mq.zero(R.st);
			mt.zero(R.st);
			cnt.zero(R.st);
			launch_expand_flags(raw.p, n, d_seed.p, n_ids, hq.p, ht.p, mq.p, mt.p, R.st);
			R.exscan(mq.p, mqs.p, n + 1);
			R.exscan(mt.p, mts.p, n + 1);
			launch_expand_count(n, file_of.p, fstart.p, hq.p, ht.p, mqs.p, mts.p, sel.p, R.st);
			launch_sel_count(sel.p, n, cnt.p, R.st);
			R.exscan(cnt.p, pos.p, n + 1);
			pos.download(&nc, 1, R.st, n);
			HIP_OK(hipStreamSynchronize(R.st));
			if (nc == 0) { hand_out(so, out, bl_id, bl_kind, n_bl); return 0; }   // (no candidate: as above)
			if (nc >= 0x7fffffffull) { fprintf(stderr, "[ndgpu_overlap] too many candidates for one sort call\n"); return -3; }
			DevBuf<OvlRec> cand(nc);
			DevBuf<uint32_t> k_span(nc), k_match(nc), k_seed(nc);
			launch_expand_write(raw.p, n, sel.p, pos.p, cand.p, k_span.p, k_match.p, k_seed.p, R.st);
			sort_and_filter(R, cand.p, k_span.p, k_match.p, k_seed.p, nc, d_seed.p, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, hq_mode, so, A, E);
		}
		const double gpu_ms = tm.stop();
		const uint64_t kept = so.n_recs, n_seeds = so.seeds;
		const double t_dev = since();
		hand_out(so, out, bl_id, bl_kind, n_bl);
		if (prof && in_core)
			fprintf(stderr, "[ndgpu_ovl_sort] %llu records: set-up %.2f ms, uploads + kernels + downloads %.2f ms, hand-out %.2f ms\n",
			        (unsigned long long)n, t_setup, t_dev - t_setup, since() - t_dev);
		if (stats) {
			stats->gpu_ms = gpu_ms, stats->raw_records = n, stats->candidates = nc, stats->seeds = n_seeds, stats->kept = kept;
			stats->ranges = n_ranges;
		}
		return (int64_t)kept;
	} catch (...) {
		return -2;
	}
}

extern "C" int64_t ndgpu_ovl_sort(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                                  uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, ndgpu_ovl_rec **out,
                                  uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats)
{
	return sort_impl(files, n_per_file, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, out, bl_id, bl_kind, n_bl, stats, false);
}

extern "C" int64_t ndgpu_ovl_sort_hq(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                                     uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, ndgpu_ovl_rec **out,
                                     uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats)
{
	return sort_impl(files, n_per_file, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, out, bl_id, bl_kind, n_bl, stats, true);
}


// Pile admission of lib/nextcorrect.py:92-143 (read_seq_data) over the records of a sorted.ovl, in file order -- host
// logic, one pass, no device work: what the stage CLI and the fused stage feed to ndgpu_correct_piles.
extern "C" int64_t ndgpu_assemble_piles(const ndgpu_ovl_rec *sorted, int64_t n, uint32_t n_ids, uint32_t min_len_seed, uint32_t min_len_aln,
                                        uint32_t max_cov_aln, uint32_t min_cov_seed, const uint32_t *skip_ids, int64_t n_skip, uint32_t **recs8,
                                        uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles)
{
	*recs8 = nullptr, *pile_off = nullptr, *seeds = nullptr, *n_piles = 0;
	std::vector<uint8_t> skip(n_ids ? n_ids : 1, 0);
	for (int64_t i = 0; i < n_skip; ++i) if (skip_ids[i] < n_ids) skip[skip_ids[i]] = 1;
	std::vector<uint32_t> used(n_ids ? n_ids : 1, 0); // stamp = group counter of the last pile that admitted the read
	std::vector<uint32_t> out;
	std::vector<uint64_t> off{0};
	std::vector<uint32_t> names;
	out.reserve((size_t)n * 8);
	const double lim = (double)max_cov_aln * 1.5;
	uint32_t stamp = 1;
	// state of the reference's loop: seed_state 0 = '' (no seed yet), 1 = valid seed, 2 = '+' (rejected seed)
	int seed_state = 0;
	uint32_t seed_name = 0;
	uint64_t total_length = 0, seed_length = 0;
	int64_t last_seed = -1;
	size_t pile_start = 0;
	auto close_pile = [&](bool keep) {
		if (keep) { off.push_back(out.size() / 8); names.push_back(seed_name); }
		else out.resize(pile_start * 8);
		pile_start = out.size() / 8;
		++stamp;
	};
	for (int64_t k = 0; k < n; ++k) {
		const ndgpu_ovl_rec &r = sorted[k]; // qname = the seed (field 0 of a sorted.ovl record), tname = the other read
		const uint32_t t_name = r.qname, t_s = r.qs, t_e = r.qe, q_name = r.tname;
		if (seed_state == 2 || (last_seed != -1 && (int64_t)t_name != last_seed)) {
			close_pile(seed_length && (double)total_length / (double)seed_length >= (double)min_cov_seed && seed_state == 1);
			seed_state = 0, total_length = seed_length = 0;
		}
		if (seed_state == 0) {
			seed_length = (uint64_t)t_e + 1;
			total_length = 0;
			seed_name = t_name;
			seed_state = (seed_length >= min_len_seed && !(t_name < n_ids && skip[t_name])) ? 1 : 2;
		}
		if (t_e - t_s < min_len_aln || (double)total_length / (double)seed_length > lim || (q_name < n_ids && used[q_name] == stamp) || seed_state == 2)
			continue;
		const uint32_t row[8] = {r.qname, r.rev, r.qs, r.qe, r.tname, r.ts, r.te, r.match};
		out.insert(out.end(), row, row + 8);
		if (q_name < n_ids) used[q_name] = stamp;
		total_length += (uint64_t)(t_e - t_s) + 1;
		last_seed = (int64_t)t_name;
	}
	close_pile(seed_length && (double)total_length / (double)seed_length >= (double)min_cov_seed && seed_state == 1);
	const size_t np = names.size(), nr = off.back();
	*recs8 = (uint32_t*)malloc(sizeof(uint32_t) * 8 * (nr ? nr : 1));
	*pile_off = (uint64_t*)malloc(sizeof(uint64_t) * (np + 1));
	*seeds = (uint32_t*)malloc(sizeof(uint32_t) * (np ? np : 1));
	if (nr) memcpy(*recs8, out.data(), sizeof(uint32_t) * 8 * nr);
	memcpy(*pile_off, off.data(), sizeof(uint64_t) * (np + 1));
	if (np) memcpy(*seeds, names.data(), sizeof(uint32_t) * np);
	*n_piles = (int64_t)np;
	return (int64_t)nr;
}


// the answer of the host routine in the place of the device's (an irregular group, or flags bit 0)
static int64_t admit_on_host(const ndgpu_ovl_rec *sorted, int64_t n, const Admission &A, const uint32_t *skip_ids, int64_t n_skip,
                             const std::vector<uint32_t> *bl, uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                             ndgpu_ovl_admit_stats *st)
{
	std::vector<uint32_t> skip(skip_ids, skip_ids + (n_skip > 0 ? n_skip : 0));
	if (bl) skip.insert(skip.end(), bl->begin(), bl->end());
	const int64_t nr = ndgpu_assemble_piles(sorted, n, A.n_ids, A.min_len_seed, A.min_len_aln, A.max_cov_aln, A.min_cov_seed, skip.data(),
	                                        (int64_t)skip.size(), recs8, pile_off, seeds, n_piles);
	st->admitted = (uint64_t)nr, st->piles = (uint64_t)*n_piles;
	return nr;
}

// the admission of `un` sorted records that lie on the device: the groups (runs of one seed id), then K16
static void admit_records(SortRun &R, const OvlRec *recs, uint64_t un, Admission &A)
{
	DevBuf<uint32_t> flag(un + 1);
	DevBuf<uint64_t> rank(un + 1);
	flag.zero(R.st);
	launch_group_flag(recs, un, flag.p, R.st);
	R.exscan(flag.p, rank.p, un + 1);
	uint64_t n_groups = 0;
	rank.download(&n_groups, 1, R.st, un);
	HIP_OK(hipStreamSynchronize(R.st));
	DevBuf<uint64_t> off(n_groups + 1);
	launch_seed_start(flag.p, rank.p, un, off.p, R.st);
	HIP_OK(hipMemcpyAsync(off.p + n_groups, &un, sizeof(un), hipMemcpyHostToDevice, R.st));
	admit_tail(R, recs, off.p, n_groups, un, A);
}

extern "C" int64_t ndgpu_admit_piles(const ndgpu_ovl_rec *sorted, int64_t n, uint32_t n_ids, uint32_t min_len_seed, uint32_t min_len_aln,
                                     uint32_t max_cov_aln, uint32_t min_cov_seed, const uint32_t *skip_ids, int64_t n_skip, int32_t flags,
                                     uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles, ndgpu_ovl_admit_stats *stats)
{
	*recs8 = nullptr, *pile_off = nullptr, *seeds = nullptr, *n_piles = 0;
	ndgpu_ovl_admit_stats st_local;
	if (!stats) stats = &st_local;
	memset(stats, 0, sizeof(*stats));
	try {
		Admission A(n_ids, min_len_seed, min_len_aln, max_cov_aln, min_cov_seed);
		if (n <= 0 || (flags & 1)) {   // nothing to admit, or the host routine asked for (the cross-check)
			A.st.sorted_records = n > 0 ? (uint64_t)n : 0;
			*stats = A.st;
			return admit_on_host(sorted, n > 0 ? n : 0, A, skip_ids, n_skip, nullptr, recs8, pile_off, seeds, n_piles, stats);
		}
		if ((uint64_t)n >= (1ull << 30)) { fprintf(stderr, "[ndgpu_overlap] too many records for one admission call\n"); return -3; }
		if (select_device(true) < 0) return -1;
		{
			SortRun R;
			HIP_OK(ndovl::create_stage_stream(&R.st));
			const StreamGuard guard{R.st};
			A.begin(skip_ids, n_skip, R.st);
			const uint64_t un = (uint64_t)n;
			DevBuf<OvlRec> recs(un);
			recs.upload((const OvlRec*)sorted, un, R.st);
			admit_records(R, recs.p, un, A);
		}
		*stats = A.st;
		if (A.declined) return admit_on_host(sorted, n, A, skip_ids, n_skip, nullptr, recs8, pile_off, seeds, n_piles, stats);
		const int64_t nr = (int64_t)A.rows.size();
		A.hand_out(recs8, pile_off, seeds, n_piles);
		return nr;
	} catch (...) {
		return -2;
	}
}

// ndgpu_ovl_sort_piles, the files as host records (files + n_per_file) or as record sets (sets)
static int64_t sort_piles_impl(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, const ndgpu_ovl_recset *const *sets, int32_t n_files,
                               const uint32_t *seed_len, uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq,
                               uint32_t min_len_seed, uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, int32_t use_bl,
                               const uint32_t *skip_ids, int64_t n_skip, int32_t flags, uint32_t **bl_id, uint8_t **bl_kind,
                               int64_t *n_bl, uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                               ndgpu_ovl_rec **sorted, int64_t *n_sorted, ndgpu_ovl_sort_stats *stats, ndgpu_ovl_admit_stats *astats)
{
	*recs8 = nullptr, *pile_off = nullptr, *seeds = nullptr, *n_piles = 0;
	if (sorted) *sorted = nullptr;
	if (n_sorted) *n_sorted = 0;
	ndgpu_ovl_admit_stats st_local;
	if (!astats) astats = &st_local;
	memset(astats, 0, sizeof(*astats));
	ndgpu_ovl_rec *srt = nullptr;
	auto drop = [&] { free(srt), free(*bl_id), free(*bl_kind); srt = nullptr, *bl_id = nullptr, *bl_kind = nullptr, *n_bl = 0; };
	try {
		Admission A(n_ids, min_len_seed, min_len_aln, max_cov_aln, min_cov_seed);
		A.use_bl = use_bl != 0;
		const bool host_only = flags & 1;
		A.want_sorted = sorted != nullptr || host_only;
		int64_t ns = sort_impl(files, n_per_file, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, &srt, bl_id, bl_kind, n_bl, stats,
		                       hq != 0, host_only ? nullptr : &A, skip_ids, n_skip, nullptr, nullptr, sets);
		if (ns < 0) return ns;
		*astats = A.st;
		if (A.declined && !A.want_sorted) {   // the sorted records were left on the device: once more, for the host routine
			drop();
			ns = sort_impl(files, n_per_file, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, &srt, bl_id, bl_kind, n_bl, stats,
			               hq != 0, nullptr, nullptr, 0, nullptr, nullptr, sets);
			if (ns < 0) return ns;
		}
		int64_t nr;
		if (A.declined || host_only) {
			astats->sorted_records = (uint64_t)ns;
			const std::vector<uint32_t> bl(*bl_id, *bl_id + *n_bl);
			nr = admit_on_host(srt, ns, A, skip_ids, n_skip, use_bl ? &bl : nullptr, recs8, pile_off, seeds, n_piles, astats);
			astats->bytes_downloaded += (uint64_t)ns * sizeof(OvlRec);
		} else {
			nr = (int64_t)A.rows.size();
			A.hand_out(recs8, pile_off, seeds, n_piles);
		}
		if (getenv("NDGPU_PROF"))
			fprintf(stderr, "[ndgpu_ovl_sort_piles] %llu sorted records in %llu groups (%llu declined, %llu wide): %llu rows in %llu piles, K16 %.3f ms, "
			        "%llu bytes downloaded\n", (unsigned long long)astats->sorted_records, (unsigned long long)astats->groups,
			        (unsigned long long)astats->groups_declined, (unsigned long long)astats->groups_wide, (unsigned long long)astats->admitted,
			        (unsigned long long)astats->piles, astats->k16_ms, (unsigned long long)astats->bytes_downloaded);
		if (sorted) *sorted = srt, srt = nullptr;
		if (n_sorted) *n_sorted = ns;
		free(srt);
		return nr;
	} catch (...) {
		drop();
		return -2;
	}
}

extern "C" int64_t ndgpu_ovl_sort_piles(const ndgpu_ovl_rec *const *files, const int64_t *n_per_file, int32_t n_files, const uint32_t *seed_len,
                                        uint32_t n_ids, int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq,
                                        uint32_t min_len_seed, uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, int32_t use_bl,
                                        const uint32_t *skip_ids, int64_t n_skip, int32_t flags, uint32_t **bl_id, uint8_t **bl_kind,
                                        int64_t *n_bl, uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                                        ndgpu_ovl_rec **sorted, int64_t *n_sorted, ndgpu_ovl_sort_stats *stats, ndgpu_ovl_admit_stats *astats)
{
	return sort_piles_impl(files, n_per_file, nullptr, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, hq, min_len_seed, min_len_aln,
	                       max_cov_aln, min_cov_seed, use_bl, skip_ids, n_skip, flags, bl_id, bl_kind, n_bl, recs8, pile_off, seeds, n_piles, sorted,
	                       n_sorted, stats, astats);
}


// ---- K17: the `.ovl` codec on the device (csrc/ovlsort_kernels.hip) ----
static bool bad_images(const uint8_t *const *bufs, const uint64_t *n_bytes, int32_t n_files)
{
	if (n_files < 0 || (n_files > 0 && (!bufs || !n_bytes))) return true;
	for (int f = 0; f < n_files; ++f) if (n_bytes[f] && !bufs[f]) return true;
	return false;
}

extern "C" int64_t ndgpu_ovl_decode_batch(const uint8_t *const *bufs, const uint64_t *n_bytes, int32_t n_files, int32_t flags, ndgpu_ovl_rec **recs,
                                          int64_t *n_per_file, uint64_t *consumed, ndgpu_ovl_codec_stats *stats)
{
	if (!recs) return -4;
	*recs = nullptr;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (bad_images(bufs, n_bytes, n_files) || (n_files > 0 && !n_per_file)) return -4;
	try {
		const ImageSet I{bufs, n_bytes, n_files};
		ndgpu_ovl_codec_stats st{};
		RecOut out;
		std::vector<int64_t> counts((size_t)n_files, 0);
		std::vector<uint64_t> used((size_t)n_files, 0);
		const uint64_t img_bytes = I.total();
		bool on_host = (flags & 1) || img_bytes == 0 || img_bytes / 8 >= 0x7fffffffull;
		if (!on_host) {
			if (select_device(true) < 0) return -1;
			SortRun R;
			HIP_OK(ndovl::create_stage_stream(&R.st));
			const StreamGuard guard{R.st};
			EvTimer tm(R.st);
			tm.start();
			DecodeRun D;
			D.count(R, I);
			if (D.total >= 0x7fffffffull) {   // (as the sort: beyond 2^31 records the call is not the device's)
				on_host = true;
				(void)tm.stop();
			} else {
				DevBuf<OvlRec> d(D.total + 1);
				D.emit(R, d.p, used.data());
				st.decode_ms = tm.stop();
				OvlRec *const dst = out.grow(D.total);
				d.download(dst, D.total, R.st);
				HIP_OK(hipStreamSynchronize(R.st));
				HIP_OK(hipGetLastError());
				counts.assign(D.n_rec.begin(), D.n_rec.end());
				st.bytes_uploaded = img_bytes, st.bytes_downloaded = D.total * sizeof(OvlRec);
			}
		}
		if (on_host) {
			decode_on_host(I, out, counts, used.data());
			if (img_bytes) st.host_decodes = (uint64_t)n_files;
		}
		st.records = out.size(), st.bytes_in = img_bytes, st.bytes_out = out.size() * sizeof(OvlRec);
		const int64_t n = (int64_t)out.size();
		*recs = (ndgpu_ovl_rec*)out.release();
		if (!*recs) throw std::runtime_error("malloc");
		for (int f = 0; f < n_files; ++f) {
			n_per_file[f] = counts[(size_t)f];
			if (consumed) consumed[f] = used[(size_t)f];
		}
		if (stats) *stats = st;
		return n;
	} catch (...) {
		return -2;
	}
}

extern "C" int64_t ndgpu_ovl_encode_batch(const ndgpu_ovl_rec *recs, int64_t n, uint32_t prev[2], int32_t flags, uint8_t **out,
                                          ndgpu_ovl_codec_stats *stats)
{
	if (!out) return -4;
	*out = nullptr;
	if (stats) memset(stats, 0, sizeof(*stats));
	if (n < 0 || !prev || (n > 0 && !recs)) return -4;
	try {
		EncodeTail E;
		E.prev[0] = prev[0], E.prev[1] = prev[1];
		if (n == 0) {
		} else if ((flags & 1) || (uint64_t)n >= 0x7fffffffull) {   // the host loop: the cross-check, and beyond 2^31 records
			uint8_t *const dst = E.image.grow((size_t)n * 40);
			const int64_t nb = ndgpu_ovl_encode(recs, n, E.prev, dst);
			E.image.n = (size_t)nb;
			E.st.bytes_out = (uint64_t)nb;
		} else {
			if (select_device(true) < 0) return -1;
			SortRun R;
			HIP_OK(ndovl::create_stage_stream(&R.st));
			const StreamGuard guard{R.st};
			DevBuf<OvlRec> d((size_t)n);
			d.upload((const OvlRec*)recs, (size_t)n, R.st);
			E.append(R, d.p, (uint64_t)n);
			E.st.bytes_uploaded = (uint64_t)n * sizeof(OvlRec);
		}
		E.st.records = (uint64_t)n, E.st.bytes_in = (uint64_t)n * sizeof(OvlRec);
		const int64_t nb = (int64_t)E.image.n;
		*out = E.image.release();
		prev[0] = E.prev[0], prev[1] = E.prev[1];
		if (stats) *stats = E.st;
		return nb;
	} catch (...) {
		return -2;
	}
}

extern "C" int64_t ndgpu_ovl_sort_images(const uint8_t *const *bufs, const uint64_t *n_bytes, int32_t n_files, const uint32_t *seed_len, uint32_t n_ids,
                                         int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq, int32_t flags, uint8_t **image,
                                         uint64_t *image_bytes, uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *sort_stats,
                                         ndgpu_ovl_codec_stats *codec_stats)
{
	if (!image || !image_bytes || !bl_id || !bl_kind || !n_bl) return -4;
	*image = nullptr, *image_bytes = 0, *bl_id = nullptr, *bl_kind = nullptr, *n_bl = 0;
	if (sort_stats) memset(sort_stats, 0, sizeof(*sort_stats));
	if (codec_stats) memset(codec_stats, 0, sizeof(*codec_stats));
	if (bad_images(bufs, n_bytes, n_files) || (n_ids > 0 && !seed_len)) return -4;
	ndgpu_ovl_rec *srt = nullptr;
	uint32_t *b_id = nullptr;
	uint8_t *b_kind = nullptr;
	int64_t nb = 0;
	try {
		const ImageSet I{bufs, n_bytes, n_files};
		EncodeTail E;
		int64_t ns;
		if (flags & 1) {   // the cross-check: the host loops around the sort as it was
			RecOut recs;
			std::vector<int64_t> counts;
			decode_on_host(I, recs, counts, nullptr);
			std::vector<const ndgpu_ovl_rec*> files;
			uint64_t at = 0;
			for (int f = 0; f < n_files; ++f) files.push_back((const ndgpu_ovl_rec*)recs.p + at), at += (uint64_t)counts[(size_t)f];
			ns = sort_impl(files.data(), counts.data(), n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, &srt, &b_id, &b_kind, &nb,
			               sort_stats, hq != 0);
			if (ns >= 0) {
				uint8_t *const dst = E.image.grow((size_t)ns * 40);
				E.image.n = (size_t)ndgpu_ovl_encode(srt, ns, E.prev, dst);
				E.st.bytes_in = I.total(), E.st.records = at, E.st.bytes_out = E.image.n, E.st.host_decodes = I.total() ? (uint64_t)n_files : 0;
			}
		} else {
			ns = sort_impl(nullptr, nullptr, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, &srt, &b_id, &b_kind, &nb, sort_stats,
			               hq != 0, nullptr, nullptr, 0, &I, &E);
		}
		free(srt), srt = nullptr;
		if (ns < 0) { free(b_id), free(b_kind); return ns; }
		const uint64_t bytes = E.image.n;
		*image = E.image.release();
		*image_bytes = bytes, *bl_id = b_id, *bl_kind = b_kind, *n_bl = nb;
		if (codec_stats) *codec_stats = E.st;
		return ns;
	} catch (...) {
		free(srt), free(b_id), free(b_kind);
		return -2;
	}
}

extern "C" int64_t ndgpu_admit_piles_image(const uint8_t *buf, uint64_t n_bytes, uint32_t n_ids, uint32_t min_len_seed, uint32_t min_len_aln,
                                           uint32_t max_cov_aln, uint32_t min_cov_seed, const uint32_t *skip_ids, int64_t n_skip, int32_t flags,
                                           uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                                           ndgpu_ovl_admit_stats *admit_stats, ndgpu_ovl_codec_stats *codec_stats)
{
	if (!recs8 || !pile_off || !seeds || !n_piles) return -4;
	*recs8 = nullptr, *pile_off = nullptr, *seeds = nullptr, *n_piles = 0;
	ndgpu_ovl_admit_stats st_local;
	if (!admit_stats) admit_stats = &st_local;
	memset(admit_stats, 0, sizeof(*admit_stats));
	if (codec_stats) memset(codec_stats, 0, sizeof(*codec_stats));
	if ((n_bytes && !buf) || n_skip < 0 || (n_skip > 0 && !skip_ids)) return -4;
	try {
		Admission A(n_ids, min_len_seed, min_len_aln, max_cov_aln, min_cov_seed);
		ndgpu_ovl_codec_stats cs{};
		const uint8_t *const bufs[1] = {buf};
		const ImageSet I{bufs, &n_bytes, 1};
		cs.bytes_in = n_bytes;
		bool on_host = (flags & 1) || n_bytes < 8 || n_bytes / 8 >= (1ull << 30);
		if (!on_host) {
			if (select_device(true) < 0) return -1;
			SortRun R;
			HIP_OK(ndovl::create_stage_stream(&R.st));
			const StreamGuard guard{R.st};
			EvTimer tm(R.st);
			tm.start();
			DecodeRun D;
			D.count(R, I);
			const uint64_t un = D.total;
			cs.bytes_uploaded = n_bytes;
			if (un >= (1ull << 30)) { fprintf(stderr, "[ndgpu_overlap] too many records for one admission call\n"); return -3; }
			if (un) {
				DevBuf<OvlRec> recs(un);
				D.emit(R, recs.p, nullptr);
				cs.decode_ms = tm.stop();
				D.release();
				A.begin(skip_ids, n_skip, R.st);
				admit_records(R, recs.p, un, A);
			}
			cs.records = un;
			on_host = A.declined;
		}
		int64_t nr;
		if (on_host) {   // flags bit 0, or a group the device form does not cover: the host loop and the host routine
			RecOut recs;
			std::vector<int64_t> counts;
			decode_on_host(I, recs, counts, nullptr);
			cs.records = recs.size(), cs.host_decodes = n_bytes ? 1 : 0;
			A.st.sorted_records = recs.size();
			*admit_stats = A.st;
			nr = admit_on_host((const ndgpu_ovl_rec*)recs.p, (int64_t)recs.size(), A, skip_ids, n_skip, nullptr, recs8, pile_off, seeds, n_piles, admit_stats);
		} else {
			*admit_stats = A.st;
			nr = (int64_t)A.rows.size();
			A.hand_out(recs8, pile_off, seeds, n_piles);
		}
		cs.bytes_out = (uint64_t)nr * 32;
		if (codec_stats) *codec_stats = cs;
		return nr;
	} catch (...) {
		return -2;
	}
}


// ---- record sets (ovl_recset.h; ndgpu_ovl_map_dev makes them in ovl_engine.hip) and K18, their stable split ----
extern "C" int64_t ndgpu_ovl_recset_size(const ndgpu_ovl_recset *set) { return set ? (int64_t)set->n : 0; }

extern "C" void ndgpu_ovl_recset_free(ndgpu_ovl_recset *set)
{
	if (!set) return;
	delete set;   // (the block goes back to the pool with the last set that shares it)
	--g_recset.sets_live;
}

extern "C" void ndgpu_ovl_recset_stats(ndgpu_ovl_recset_counters *out, int reset)
{
	RecsetCounters &c = g_recset;
	if (out) {
		out->split_ms = (double)c.split_ns.load() * 1e-6;
		out->sets_made = c.sets_made, out->sets_live = c.sets_live, out->bytes_downloaded = c.bytes_downloaded, out->bytes_uploaded = c.bytes_uploaded;
		out->bytes_d2d = c.bytes_d2d, out->split_calls = c.split_calls, out->sets_downloaded = c.sets_downloaded;
	}
	if (reset) c.split_ns = 0, c.sets_made = 0, c.bytes_downloaded = 0, c.bytes_uploaded = 0, c.bytes_d2d = 0, c.split_calls = 0, c.sets_downloaded = 0;
}

extern "C" int64_t ndgpu_ovl_recset_download(const ndgpu_ovl_recset *set, ndgpu_ovl_rec *out, int64_t cap)
{
	const uint64_t n = set ? set->n : 0;
	if (cap < 0 || (uint64_t)cap < n || (n && !out)) return -4;
	if (!n) return 0;
	try {
		if (select_device(true) < 0) return -1;
		SortRun R;
		HIP_OK(ndovl::create_stage_stream(&R.st));
		const StreamGuard guard{R.st};
		HIP_OK(hipMemcpyAsync(out, set->data(), n * sizeof(OvlRec), hipMemcpyDeviceToHost, R.st));
		HIP_OK(hipStreamSynchronize(R.st));
		g_recset.bytes_downloaded += n * sizeof(OvlRec);
		return (int64_t)n;
	} catch (...) {
		return -2;
	}
}

extern "C" ndgpu_ovl_recset *ndgpu_ovl_recset_upload(const ndgpu_ovl_rec *recs, int64_t n)
{
	if (n < 0 || (n > 0 && !recs)) return nullptr;
	try {
		if (n == 0) return recset_view(nullptr, 0, 0);
		if (select_device(true) < 0) return nullptr;
		SortRun R;
		HIP_OK(ndovl::create_stage_stream(&R.st));
		const StreamGuard guard{R.st};
		DevBuf<OvlRec> d((size_t)n);
		d.upload((const OvlRec*)recs, (size_t)n, R.st);
		HIP_OK(hipStreamSynchronize(R.st));
		g_recset.bytes_uploaded += (uint64_t)n * sizeof(OvlRec);
		return recset_own(std::move(d), (uint64_t)n);
	} catch (...) {
		return nullptr;
	}
}

extern "C" ndgpu_ovl_recset *ndgpu_ovl_recset_concat(const ndgpu_ovl_recset *const *sets, int32_t n)
{
	if (n < 0 || (n > 0 && !sets)) return nullptr;
	try {
		uint64_t total = 0;
		for (int f = 0; f < n; ++f) total += sets[f] ? sets[f]->n : 0;
		if (total == 0) return recset_view(nullptr, 0, 0);
		if (select_device(true) < 0) return nullptr;
		SortRun R;
		HIP_OK(ndovl::create_stage_stream(&R.st));
		const StreamGuard guard{R.st};
		DevBuf<OvlRec> d(total);
		uint64_t at = 0;
		for (int f = 0; f < n; ++f) {
			const uint64_t m = sets[f] ? sets[f]->n : 0;
			if (m) HIP_OK(hipMemcpyAsync(d.p + at, sets[f]->data(), m * sizeof(OvlRec), hipMemcpyDeviceToDevice, R.st));
			at += m;
		}
		HIP_OK(hipStreamSynchronize(R.st));
		g_recset.bytes_d2d += total * sizeof(OvlRec);
		return recset_own(std::move(d), total);
	} catch (...) {
		return nullptr;
	}
}

// K18: count per (file, tile), one scan over the table in file-major order, the cut points, scatter.  The output sets are views into
// one block.
extern "C" int64_t ndgpu_ovl_recset_split(const ndgpu_ovl_recset *set, const uint32_t *file_of, uint32_t n_ids, int32_t n_files,
                                          ndgpu_ovl_recset **out_sets)
{
	if (!out_sets || n_files <= 0) return -4;
	for (int f = 0; f < n_files; ++f) out_sets[f] = nullptr;
	const uint64_t n = set ? set->n : 0;
	if ((uint32_t)n_files > split_max_files() || (n_ids > 0 && !file_of)) return -4;
	try {
		if (n == 0) {
			for (int f = 0; f < n_files; ++f) out_sets[f] = recset_view(nullptr, 0, 0);
			return 0;
		}
		if (select_device(true) < 0) return -1;
		SortRun R;
		HIP_OK(ndovl::create_stage_stream(&R.st));
		const StreamGuard guard{R.st};
		EvTimer tm(R.st);
		tm.start();
		const uint64_t tile = split_tile_records(), n_tiles = (n + tile - 1) / tile;
		if (n_tiles >= 0x7fffffffull) throw std::runtime_error("too many records for one split call");
		const size_t cells = (size_t)n_tiles * (size_t)n_files;
		DevBuf<uint32_t> d_file(n_ids), cnt(cells + 1), bad(1);
		DevBuf<uint64_t> first(cells + 1), cuts((size_t)n_files + 1);
		d_file.upload(file_of, n_ids, R.st);
		bad.zero(R.st);
		HIP_OK(hipMemsetAsync(cnt.p + cells, 0, sizeof(uint32_t), R.st));   // (the scan's last entry = all rows)
		launch_split_count(set->data(), n, d_file.p, n_ids, (uint32_t)n_files, n_tiles, cnt.p, bad.p, R.st);
		R.exscan(cnt.p, first.p, cells + 1);
		launch_split_cuts(first.p, n_tiles, (uint32_t)n_files, cuts.p, R.st);
		std::vector<uint64_t> h_cuts((size_t)n_files + 1);
		uint32_t h_bad = 0;
		cuts.download(h_cuts.data(), (size_t)n_files + 1, R.st);
		bad.download(&h_bad, 1, R.st);
		HIP_OK(hipStreamSynchronize(R.st));   // (file_of, the caller's array, has been read)
		HIP_OK(hipGetLastError());
		++g_recset.split_calls;
		if (h_bad) {   // a record that belongs to no file: no set is made
			g_recset.split_ns += (uint64_t)(tm.stop() * 1e6);
			fprintf(stderr, "[ndgpu_overlap] ndgpu_ovl_recset_split: %u records whose query read is in none of the %d files\n", h_bad, n_files);
			return -2;
		}
		if (h_cuts[0] != 0 || h_cuts[(size_t)n_files] != n) throw std::runtime_error("split counts out of range");
		auto out = std::make_shared<DevBuf<OvlRec>>((size_t)n);
		launch_split_scatter(set->data(), n, d_file.p, n_ids, (uint32_t)n_files, n_tiles, first.p, out->p, R.st);
		g_recset.split_ns += (uint64_t)(tm.stop() * 1e6);   // (waits for the stream)
		HIP_OK(hipGetLastError());
		g_recset.bytes_d2d += n * sizeof(OvlRec);
		for (int f = 0; f < n_files; ++f) out_sets[f] = recset_view(out, h_cuts[(size_t)f], h_cuts[(size_t)f + 1] - h_cuts[(size_t)f]);
		return 0;
	} catch (...) {
		for (int f = 0; f < n_files; ++f) ndgpu_ovl_recset_free(out_sets[f]), out_sets[f] = nullptr;
		return -2;
	}
}

extern "C" int64_t ndgpu_ovl_sort_sets(const ndgpu_ovl_recset *const *files, int32_t n_files, const uint32_t *seed_len, uint32_t n_ids,
                                       int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq, ndgpu_ovl_rec **out,
                                       uint32_t **bl_id, uint8_t **bl_kind, int64_t *n_bl, ndgpu_ovl_sort_stats *stats)
{
	return sort_impl(nullptr, nullptr, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, out, bl_id, bl_kind, n_bl, stats, hq != 0,
	                 nullptr, nullptr, 0, nullptr, nullptr, files);
}

extern "C" int64_t ndgpu_ovl_sort_piles_sets(const ndgpu_ovl_recset *const *files, int32_t n_files, const uint32_t *seed_len, uint32_t n_ids,
                                             int32_t min_seed_len, int32_t max_bin_cov, int32_t max_flank_len, int32_t hq, uint32_t min_len_seed,
                                             uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, int32_t use_bl,
                                             const uint32_t *skip_ids, int64_t n_skip, int32_t flags, uint32_t **bl_id, uint8_t **bl_kind,
                                             int64_t *n_bl, uint32_t **recs8, uint64_t **pile_off, uint32_t **seeds, int64_t *n_piles,
                                             ndgpu_ovl_rec **sorted, int64_t *n_sorted, ndgpu_ovl_sort_stats *stats, ndgpu_ovl_admit_stats *astats)
{
	return sort_piles_impl(nullptr, nullptr, files, n_files, seed_len, n_ids, min_seed_len, max_bin_cov, max_flank_len, hq, min_len_seed, min_len_aln,
	                       max_cov_aln, min_cov_seed, use_bl, skip_ids, n_skip, flags, bl_id, bl_kind, n_bl, recs8, pile_off, seeds, n_piles, sorted,
	                       n_sorted, stats, astats);
}

// ---- K23: the step-2 writer on the device (kernels: ovlsort_kernels.hip; the run's state and the C entry: ovl_step2.cpp) ----
namespace {
struct S2Dev {
	SortRun R;
	EvTimer *tm = nullptr;
	uint32_t n = 0, d = 0;
	uint64_t m = 0;
	DevBuf<OvlRec10> recs;
	DevBuf<uint32_t> skey, sval, rinfo, flagw, seg_start, seg_name, seg_first, segof;
	~S2Dev()   // the stream ends before the buffers go back to the pool
	{
		if (R.st) { (void)hipStreamSynchronize(R.st); delete tm; (void)hipStreamDestroy(R.st); }
		R.tmp.buf.release();
	}
};
// declared behind a step's buffers: whatever still runs when the step fails has finished before they go back to the pool
struct S2Sync { hipStream_t s; ~S2Sync() { (void)hipStreamSynchronize(s); } };
}

namespace ndovl {

void s2_group(S2Call &c)
{
	if (select_device(true) < 0) throw std::runtime_error("no device");
	S2Dev *D = new S2Dev();
	c.dev = D;
	HIP_OK(create_stage_stream(&D->R.st));
	hipStream_t st = D->R.st;
	D->tm = new EvTimer(st);
	D->tm->start();
	const uint32_t n = D->n = c.n;
	const uint64_t m = D->m = 2 * (uint64_t)n;
	D->recs.alloc(n), D->rinfo.alloc(n), D->flagw.alloc(2);
	D->skey.alloc(m), D->sval.alloc(m), D->segof.alloc(m);
	D->seg_start.alloc(m + 1), D->seg_name.alloc(m + 1), D->seg_first.alloc(m + 1);
	D->recs.upload(c.recs, n, st);
	D->flagw.zero(st);
	c.bytes_up += (uint64_t)n * sizeof(OvlRec10);
	uint64_t d64 = 0;
	{
		DevBuf<uint32_t> ekey, eval, head;
		DevBuf<uint64_t> rank;
		const S2Sync sync{st};
		ekey.alloc(m), eval.alloc(m), head.alloc(m + 1), rank.alloc(m + 1);
		launch_s2_classify(D->recs.p, n, c.h2, ekey.p, eval.p, D->rinfo.p, D->flagw.p, st);
		D->R.tmp.run([&](void *t, size_t &tb) { sort_pairs_u32(t, tb, ekey.p, D->skey.p, eval.p, D->sval.p, m, st); });   // stable: record order inside a read
		launch_s2_segments(D->skey.p, D->sval.p, m, head.p, rank.p, false, nullptr, nullptr, nullptr, nullptr, st);
		D->R.exscan(head.p, rank.p, m + 1);
		launch_s2_segments(D->skey.p, D->sval.p, m, head.p, rank.p, true, D->seg_start.p, D->seg_name.p, D->seg_first.p, D->segof.p, st);
		c.launches += 5;
		rank.download(&d64, 1, st, m);
		D->flagw.download(&c.decline, 1, st);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		c.bytes_down += 12;
	}
	if (c.decline) { c.ms += D->tm->stop(); return; }
	const uint32_t d = D->d = (uint32_t)d64;
	c.name.resize(d), c.first.resize(d), c.order.resize(d);
	{
		DevBuf<uint32_t> idx, key2, ord;
		const S2Sync sync{st};
		idx.alloc(d), key2.alloc(d), ord.alloc(d);
		launch_iota(idx.p, d, st);
		D->R.tmp.run([&](void *t, size_t &tb) { sort_pairs_u32(t, tb, D->seg_first.p, key2.p, idx.p, ord.p, d, st); });
		c.launches += 2;
		D->seg_name.download(c.name.data(), d, st);
		D->seg_first.download(c.first.data(), d, st);
		ord.download(c.order.data(), d, st);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		c.bytes_down += 12ull * d;
	}
	c.ms += D->tm->stop();
}

void s2_solve(S2Call &c)
{
	S2Dev *D = (S2Dev*)c.dev;
	hipStream_t st = D->R.st;
	const uint32_t n = D->n, d = D->d;
	const uint64_t m = D->m;
	DevBuf<uint32_t> con0, alive_a, alive_b, con, einfo, keptw, kidx, len, n_alive, n_merged;
	DevBuf<uint8_t> kept, bytes;
	DevBuf<uint64_t> krank, boff, ioff, moff, key, val, key2, val2;
	DevBuf<S2ReadOut> out;
	DevBuf<uint2> merged, dense;
	const S2Sync sync{st};
	D->tm->start();
	con0.alloc(d), alive_a.alloc(d), alive_b.alloc(d), con.alloc(d);
	con0.upload(c.con0.data(), d, st);
	c.bytes_up += 4ull * d;
	launch_s2_init(con0.p, d, alive_a.p, st);
	c.launches++;
	uint32_t *cur = alive_a.p, *nxt = alive_b.p;
	c.converged = false;
	while (c.rounds < c.max_rounds) {
		uint32_t changed = 0;
		HIP_OK(hipMemsetAsync(D->flagw.p + 1, 0, sizeof(uint32_t), st));
		launch_s2_events(D->seg_start.p, d, D->sval.p, D->rinfo.p, D->segof.p, con0.p, cur, nxt, con.p, D->flagw.p + 1, st);
		D->flagw.download(&changed, 1, st, 1);
		HIP_OK(hipStreamSynchronize(st));
		HIP_OK(hipGetLastError());
		c.launches++, c.rounds++, c.bytes_down += 4;
		std::swap(cur, nxt);
		if (!changed) { c.converged = true; break; }
	}
	if (!c.converged) { c.ms += D->tm->stop(); return; }

	// the verdicts and the encoder's plan
	einfo.alloc(m), keptw.alloc((size_t)n + 1), kidx.alloc(n), len.alloc((size_t)n + 1), kept.alloc(n);
	krank.alloc((size_t)n + 1), boff.alloc((size_t)n + 1);
	launch_s2_verdict(D->recs.p, n, c.h1, c.h2, D->rinfo.p, D->segof.p, cur, einfo.p, keptw.p, kept.p, st);
	D->R.exscan(keptw.p, krank.p, (size_t)n + 1);
	launch_s2_compact(keptw.p, krank.p, n, kidx.p, st);
	launch_s2_size10(D->recs.p, kidx.p, krank.p, n, c.prev[0], c.prev[1], len.p, st);
	D->R.exscan(len.p, boff.p, (size_t)n + 1);
	// the reads: counts and maxima, then the union of their intervals
	out.alloc(d), n_alive.alloc((size_t)d + 1), n_merged.alloc((size_t)d + 1), ioff.alloc((size_t)d + 1), moff.alloc((size_t)d + 1);
	key.alloc(m), val.alloc(m), key2.alloc(m), val2.alloc(m), merged.alloc(m);
	launch_s2_reduce(D->seg_start.p, d, D->sval.p, einfo.p, D->recs.p, con.p, out.p, n_alive.p, st);
	D->R.exscan(n_alive.p, ioff.p, (size_t)d + 1);
	launch_s2_span_keys(D->sval.p, m, D->segof.p, einfo.p, con.p, D->recs.p, key.p, val.p, st);
	unsigned bits = 1;
	while (bits < 32 && (d >> bits)) ++bits;   // d < 2^bits: a live key's read field is never all ones, the keys of dead entries sort last
	D->R.tmp.run([&](void *t, size_t &tb) { sort_pairs_u64(t, tb, key.p, key2.p, val.p, val2.p, m, 0, 32 + bits, st); });
	launch_s2_union(ioff.p, d, key2.p, val2.p, merged.p, n_merged.p, st);
	D->R.exscan(n_merged.p, moff.p, (size_t)d + 1);
	c.launches += 11;
	uint64_t nk = 0, nb = 0, ns = 0;
	krank.download(&nk, 1, st, n);
	boff.download(&nb, 1, st, n);
	moff.download(&ns, 1, st, d);
	HIP_OK(hipStreamSynchronize(st));
	HIP_OK(hipGetLastError());
	if (nk > n || nb > 47 * nk || nb < 10 * nk || ns > m) throw std::runtime_error("step-2 sizes out of range");

	bytes.alloc(nb + 4), dense.alloc(ns);
	launch_s2_write10(D->recs.p, kidx.p, nk, c.prev[0], c.prev[1], boff.p, bytes.p, st);
	launch_s2_span_gather(ioff.p, moff.p, d, n_merged.p, merged.p, dense.p, st);
	c.launches += 2;
	c.con.resize(d), c.out.resize(d), c.span_off.resize((size_t)d + 1), c.spans.resize(ns);
	c.bytes = (uint8_t*)malloc(nb ? nb : 1);
	if (!c.bytes) throw std::runtime_error("malloc");
	uint32_t last = 0;
	con.download(c.con.data(), d, st);
	out.download(c.out.data(), d, st);
	moff.download(c.span_off.data(), (size_t)d + 1, st);
	dense.download(c.spans.data(), ns, st);
	bytes.download(c.bytes, nb, st);
	if (c.kept) kept.download(c.kept, n, st);
	if (nk) kidx.download(&last, 1, st, nk - 1);
	c.ms += D->tm->stop();   // (waits for the downloads)
	HIP_OK(hipStreamSynchronize(st));
	HIP_OK(hipGetLastError());
	c.bytes_down += 24 + 4ull * d + sizeof(S2ReadOut) * (uint64_t)d + 8ull * (d + 1) + 8 * ns + nb + (c.kept ? n : 0) + (nk ? 4 : 0);
	c.n_bytes = nb, c.n_kept = nk;
	c.prev_out[0] = nk ? c.recs[last].qname : c.prev[0], c.prev_out[1] = nk ? c.recs[last].tname : c.prev[1];
}

void s2_release(S2Call &c)
{
	delete (S2Dev*)c.dev;
	c.dev = nullptr;
	free(c.bytes);
	c.bytes = nullptr;
}

} // namespace ndovl
