// ovlsort_kernels.hip -- gfx950 kernels of the overlap sort / filter stage (util/ovl_sort.c path, raw reads).
//
//   S1 expand_flags / expand_write   step-1 records -> per-seed candidates in both directions
//                                    (ovl_sort.c:980-1037: pre-filters, seed lookup, "5 misses then stop" per file)
//   S2 rocPRIM LSD radix sorts       order (seed asc, match desc, span asc), stable (ovl_sort.c:246-261, 876-925)
//   S3 seed_filter_kernel            one wavefront per seed: 64-base coverage bins in LDS, candidates admitted
//                                    one after the other (ovl_sort.c:675-741), then the chimera / low-coverage
//                                    trimming and the .bl verdict (ovl_sort.c:316-383, 433-571)
// HBM/LDS integer work; the admission chain is sequential per seed, seeds are independent.
#include <cstring>
#include <hip/hip_runtime.h>
#include <rocprim/rocprim.hpp>

#include "ovl_device.h"

namespace ndovl {

constexpr int kBinShift = 6;

__global__ void expand_flags_kernel(const OvlRec *__restrict__ raw, uint64_t n, const uint32_t *__restrict__ seed_len, uint32_t n_ids,
                                    uint32_t *__restrict__ hit_q, uint32_t *__restrict__ hit_t, uint32_t *__restrict__ miss_q,
                                    uint32_t *__restrict__ miss_t)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const OvlRec r = raw[i];
	uint32_t hq = 0, ht = 0, mq = 0, mt = 0;
	if (!(r.qname == r.tname || r.qe - r.qs < 500 || r.te - r.ts < 500)) {
		hq = r.qname < n_ids && seed_len[r.qname] && seed_len[r.qname] >= r.qe;
		ht = r.tname < n_ids && seed_len[r.tname] && seed_len[r.tname] >= r.te;
		mq = !hq, mt = !ht;
	}
	hit_q[i] = hq, hit_t[i] = ht, miss_q[i] = mq, miss_t[i] = mt;
}

// file_of[i] = input file of record i; miss_*_scan = exclusive scans over all records; file_start[f] = first record of file f
__global__ void expand_count_kernel(uint64_t n, const uint32_t *__restrict__ file_of, const uint64_t *__restrict__ file_start,
                                    const uint32_t *__restrict__ hit_q, const uint32_t *__restrict__ hit_t,
                                    const uint64_t *__restrict__ miss_q_scan, const uint64_t *__restrict__ miss_t_scan,
                                    uint32_t *__restrict__ n_out)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint64_t f0 = file_start[file_of[i]];
	// a side stops being collected once 5 of its records in this file missed the seed table
	const bool q = hit_q[i] && miss_q_scan[i] - miss_q_scan[f0] < 5;
	const bool t = hit_t[i] && miss_t_scan[i] - miss_t_scan[f0] < 5;
	n_out[i] = (uint32_t)q | (uint32_t)t << 1;
}

__global__ void expand_write_kernel(const OvlRec *__restrict__ raw, uint64_t n, const uint32_t *__restrict__ sel, const uint64_t *__restrict__ pos,
                                    OvlRec *__restrict__ cand, uint32_t *__restrict__ k_span, uint32_t *__restrict__ k_match,
                                    uint32_t *__restrict__ k_seed)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = sel[i];
	if (!s) return;
	const OvlRec r = raw[i];
	uint64_t o = pos[i];
	if (s & 1) {
		OvlRec c;
		c.rev = r.rev, c.qname = r.qname, c.qs = r.qs, c.qe = r.qe - 1, c.tname = r.tname, c.ts = r.ts, c.te = r.te - 1, c.match = r.match;
		cand[o] = c;
		k_span[o] = c.qe - c.qs, k_match[o] = ~c.match, k_seed[o] = c.qname;
		++o;
	}
	if (s & 2) {
		OvlRec c;
		c.rev = r.rev, c.qname = r.tname, c.qs = r.ts, c.qe = r.te - 1, c.tname = r.qname, c.ts = r.qs, c.te = r.qe - 1, c.match = r.match;
		cand[o] = c;
		k_span[o] = c.qe - c.qs, k_match[o] = ~c.match, k_seed[o] = c.qname;
	}
}

__global__ void sel_count_kernel(const uint32_t *__restrict__ sel, uint64_t n, uint32_t *__restrict__ cnt)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) cnt[i] = (sel[i] & 1) + (sel[i] >> 1 & 1);
}

__global__ void iota_kernel(uint32_t *__restrict__ a, uint64_t n)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) a[i] = (uint32_t)i;
}

__global__ void gather_u32_kernel(const uint32_t *__restrict__ src, const uint32_t *__restrict__ idx, uint64_t n, uint32_t *__restrict__ dst)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) dst[i] = src[idx[i]];
}

// seed boundaries in sorted order: flag[i] = 1 where a new seed starts
__global__ void seed_flag_kernel(const OvlRec *__restrict__ cand, const uint32_t *__restrict__ perm, uint64_t n, uint32_t *__restrict__ flag)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) flag[i] = i == 0 || cand[perm[i]].qname != cand[perm[i - 1]].qname;
}

__global__ void seed_start_kernel(const uint32_t *__restrict__ flag, const uint64_t *__restrict__ rank, uint64_t n, uint64_t *__restrict__ start)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && flag[i]) start[rank[i]] = i;
}

#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)
// ---- the out-of-core form (csrc/ovlsort_engine.hip: sort_out_of_core): the records of ONE file arrive in pieces ----
// like expand_count_kernel for a piece of one file: carry_* = records of this file before the piece that missed the seed table
__global__ void expand_count_piece_kernel(uint64_t n, const uint32_t *__restrict__ hit_q, const uint32_t *__restrict__ hit_t,
                                          const uint64_t *__restrict__ miss_q_scan, const uint64_t *__restrict__ miss_t_scan, uint64_t carry_q,
                                          uint64_t carry_t, uint32_t *__restrict__ sel)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const bool q = hit_q[i] && carry_q + miss_q_scan[i] < 5;
	const bool t = hit_t[i] && carry_t + miss_t_scan[i] < 5;
	sel[i] = (uint32_t)q | (uint32_t)t << 1;
}

// candidates per seed (which seed ranges fit the device at a time)
__global__ void cand_hist_kernel(const OvlRec *__restrict__ raw, const uint32_t *__restrict__ sel, uint64_t n, uint32_t *__restrict__ hist)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = sel[i];
	if (s & 1) atomicAdd(hist + raw[i].qname, 1u);
	if (s & 2) atomicAdd(hist + raw[i].tname, 1u);
}

// the sides of a record whose seed lies in [lo, hi)
__global__ void range_sel_kernel(const OvlRec *__restrict__ raw, const uint8_t *__restrict__ sel, uint64_t n, uint32_t lo, uint32_t hi,
                                 uint32_t *__restrict__ out)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t s = sel[i];
	const OvlRec r = raw[i];
	out[i] = (uint32_t)((s & 1) && r.qname >= lo && r.qname < hi) | (uint32_t)((s & 2) && r.tname >= lo && r.tname < hi) << 1;
}

__global__ void narrow_u32_u8_kernel(const uint32_t *__restrict__ in, uint64_t n, uint8_t *__restrict__ out)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = (uint8_t)in[i];
}


void launch_expand_flags(const OvlRec *raw, uint64_t n, const uint32_t *seed_len, uint32_t n_ids, uint32_t *hq, uint32_t *ht, uint32_t *mq,
                         uint32_t *mt, hipStream_t s)
{
	if (n) ND_LAUNCH(expand_flags_kernel, GRID1(n), 0, s, raw, n, seed_len, n_ids, hq, ht, mq, mt);
}
void launch_expand_count(uint64_t n, const uint32_t *file_of, const uint64_t *file_start, const uint32_t *hq, const uint32_t *ht,
                         const uint64_t *mqs, const uint64_t *mts, uint32_t *sel, hipStream_t s)
{
	if (n) ND_LAUNCH(expand_count_kernel, GRID1(n), 0, s, n, file_of, file_start, hq, ht, mqs, mts, sel);
}
void launch_expand_count_piece(uint64_t n, const uint32_t *hq, const uint32_t *ht, const uint64_t *mqs, const uint64_t *mts, uint64_t carry_q,
                               uint64_t carry_t, uint32_t *sel, hipStream_t s)
{
	if (n) ND_LAUNCH(expand_count_piece_kernel, GRID1(n), 0, s, n, hq, ht, mqs, mts, carry_q, carry_t, sel);
}
void launch_cand_hist(const OvlRec *raw, const uint32_t *sel, uint64_t n, uint32_t *hist, hipStream_t s)
{
	if (n) ND_LAUNCH(cand_hist_kernel, GRID1(n), 0, s, raw, sel, n, hist);
}
void launch_range_sel(const OvlRec *raw, const uint8_t *sel, uint64_t n, uint32_t lo, uint32_t hi, uint32_t *out, hipStream_t s)
{
	if (n) ND_LAUNCH(range_sel_kernel, GRID1(n), 0, s, raw, sel, n, lo, hi, out);
}
void launch_narrow_u32_u8(const uint32_t *in, uint64_t n, uint8_t *out, hipStream_t s)
{
	if (n) ND_LAUNCH(narrow_u32_u8_kernel, GRID1(n), 0, s, in, n, out);
}
void launch_sel_count(const uint32_t *sel, uint64_t n, uint32_t *cnt, hipStream_t s)
{
	if (n) ND_LAUNCH(sel_count_kernel, GRID1(n), 0, s, sel, n, cnt);
}
void launch_expand_write(const OvlRec *raw, uint64_t n, const uint32_t *sel, const uint64_t *pos, OvlRec *cand, uint32_t *k_span,
                         uint32_t *k_match, uint32_t *k_seed, hipStream_t s)
{
	if (n) ND_LAUNCH(expand_write_kernel, GRID1(n), 0, s, raw, n, sel, pos, cand, k_span, k_match, k_seed);
}
void launch_iota(uint32_t *a, uint64_t n, hipStream_t s) { if (n) ND_LAUNCH(iota_kernel, GRID1(n), 0, s, a, n); }
void launch_gather_u32(const uint32_t *src, const uint32_t *idx, uint64_t n, uint32_t *dst, hipStream_t s)
{
	if (n) ND_LAUNCH(gather_u32_kernel, GRID1(n), 0, s, src, idx, n, dst);
}
void launch_seed_flag(const OvlRec *cand, const uint32_t *perm, uint64_t n, uint32_t *flag, hipStream_t s)
{
	if (n) ND_LAUNCH(seed_flag_kernel, GRID1(n), 0, s, cand, perm, n, flag);
}
void launch_seed_start(const uint32_t *flag, const uint64_t *rank, uint64_t n, uint64_t *start, hipStream_t s)
{
	if (n) ND_LAUNCH(seed_start_kernel, GRID1(n), 0, s, flag, rank, n, start);
}

void sort_pairs_u32(void *tmp, size_t &tmp_bytes, const uint32_t *kin, uint32_t *kout, const uint32_t *vin, uint32_t *vout, size_t n,
                   hipStream_t s)
{
	if (tmp && fault_injected()) device_check((int)hipErrorOutOfMemory, __func__);
	device_check((int)rocprim::radix_sort_pairs(tmp, tmp_bytes, kin, kout, vin, vout, n, 0, 32, s), __func__);
}

// ------------------------------------------------------------------------------------------------
// S3: one wavefront per seed

__device__ __forceinline__ int wave_sum(int v) { for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64); return v; }
__device__ __forceinline__ int wave_min(int v) { for (int d = 32; d; d >>= 1) { int o = __shfl_xor(v, d, 64); v = o < v ? o : v; } return v; }

constexpr uint32_t kSelf = 0x7fffffffu;  // kept[] entry of the synthetic self record
constexpr uint32_t kDropped = 0x80000000u;

__global__ void __launch_bounds__(64) seed_filter_kernel(const OvlRec *__restrict__ cand, const uint32_t *__restrict__ perm,
                                                          const uint64_t *__restrict__ seed_start, uint32_t n_seeds, uint64_t n_cand,
                                                          const uint32_t *__restrict__ seed_len, int max_bin_cov, int flank, int min_seed_len,
                                                          uint32_t max_bins, uint32_t *__restrict__ kept, OvlRec *__restrict__ out,
                                                          uint32_t *__restrict__ n_out, uint32_t *__restrict__ bl_id, uint8_t *__restrict__ bl_kind)
{
	extern __shared__ uint16_t bins[];
	const uint32_t sd = blockIdx.x;
	if (sd >= n_seeds) return;
	const int lane = threadIdx.x;
	const uint64_t c0 = seed_start[sd], c1 = sd + 1 < n_seeds ? seed_start[sd + 1] : n_cand;
	const uint32_t seed = cand[perm[c0]].qname;
	const uint32_t qlen = seed_len[seed];
	const int nb = (int)(qlen >> kBinShift) + 1;
	uint32_t *K = kept + c0 + sd;       // room for the self record + every candidate of the seed
	OvlRec *O = out + c0 + sd;
	for (int i = lane; i < nb && i < (int)max_bins; i += 64) bins[i] = 0;
	__syncthreads();

	// state of the admission chain (identical in every lane)
	uint8_t repeat_run = 1;
	uint32_t n_kept = 0, last_qs = 0, last_qe = qlen - 1, qcov = qlen, bins_touched = 0, bins_sum = 0, contained = 0;
	const uint32_t qcap = qlen * 150u;
	if (lane == 0) K[0] = kSelf;
	n_kept = 1;
	for (uint64_t c = c0; c < c1; ++c) {
		const uint32_t ci = perm[c];
		const OvlRec o = cand[ci];
		if (qcov > qcap || n_kept > 65535u - 1000u) continue;
		const int j = (int)((o.qs + 10) >> kBinShift), k = (int)((o.qe - 10) >> kBinShift);
		int label = 1;
		const int dqs = (int)(o.qs - last_qs), dqe = (int)(o.qe - last_qe);
		if ((j > 15 || k < nb - 16) && (dqs < 0 ? -dqs : dqs) < 50 && (dqe < 0 ? -dqe : dqe) < 50) label = repeat_run++ < 5 ? 2 : 0;
		if (!label) continue;
		int fresh = 0, lowest = 200, sum = 0;
		for (int i = j + 1 + lane; i <= k; i += 64) {
			int v = bins[i];
			if (!v) ++fresh;
			++v;
			if (v < lowest) lowest = v;
			if (v > 65535 - 1000) --v;
			bins[i] = (uint16_t)v;
			sum += v;
		}
		fresh = wave_sum(fresh), sum = wave_sum(sum), lowest = wave_min(lowest);
		// float quotients of the reference, formed in double and rounded once (exact for 24-bit operands)
		const float lhs = (float)((double)(float)sum / (double)(float)(k - j));
		const float dens = (float)((double)(float)bins_sum / (double)(float)bins_touched);
		const float clampd = dens > 10 ? dens : 10;                      // max(dens, 10) of the reference's macro
		const float lim = clampd > max_bin_cov ? (float)max_bin_cov : clampd; // min(.., max_bin_cov)
		const bool reject = (lowest > max_bin_cov || (double)lhs > 1.3 * (double)lim) && ((double)(o.qe - o.qs) <= qlen * 0.8);
		if (reject) {
			for (int i = j + 1 + lane; i <= k; i += 64) bins[i]--;
			ND_LOCKSTEP();  // the next record's lanes own other bins
			continue;
		}
		if (label != 2) repeat_run = 1;
		bins_touched += (uint32_t)fresh;
		bins_sum += (uint32_t)(k - j);
		last_qs = o.qs, last_qe = o.qe;
		qcov += o.qe - o.qs + 1;
		if (o.qname != o.tname && o.qs <= (uint32_t)flank && o.qe + (uint32_t)flank >= qlen) ++contained;
		if (lane == 0) K[n_kept] = ci;
		++n_kept;
	}
	__syncthreads();

	// end of the seed (lane 0 walks the bins; the few list scans are short)
	uint32_t chimera = 0;
	int lo = 0, hi = 0;
	if (lane == 0) {
		// coverage-shape chimera test
		{
			int label = 0, ll = 0, rl = 0;
			for (int i = 1; i < nb - 1; ++i) {
				if (bins[i] > 20 && ++ll) {
					if (label && ++rl >= 5) break;
				} else {
					const int l = i - 5 > 0 ? i - 5 : 0, r = i + 5 > nb - 1 ? nb - 1 : i + 5;
					const int mn = bins[l] > bins[r] ? bins[r] : bins[l];
					if (ll > 5 && (bins[l] > 20 || bins[r] > 20) && bins[i] <= (3 > mn / 5 ? 3 : mn / 5)) label = i;
				}
			}
			if (rl < 5) label = 0;
			chimera = (uint32_t)label;
		}
		if (chimera || !contained) {
			int j = 0;
			uint16_t *b = bins; // (first, last) pairs of low-coverage bin runs overwrite the front of bins[]
			if (qcov > qlen * 10u) {
				const int low = 4 > max_bin_cov / 10 ? max_bin_cov / 10 : 4;
				for (int i = 1; i < nb - 1; ++i) {
					if (b[i] < low) {
						if (lo == 0) lo = i;
						hi = i;
					} else if (lo) {
						if (chimera && chimera < (uint32_t)lo && ((!j) || chimera > b[j - 1])) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
						b[j++] = (uint16_t)lo, b[j++] = (uint16_t)hi;
						lo = hi = 0;
					}
				}
				if (lo) {
					if (chimera && chimera < (uint32_t)lo && ((!j) || chimera > b[j - 1])) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
					b[j++] = (uint16_t)lo, b[j++] = (uint16_t)hi;
				}
				if (chimera && (j == 0 || chimera > b[j - 1])) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
			} else if (chimera) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
			if (j) {
				int m = j, k = 0, i;
				if (b[0] < 5) m -= 2;
				if (b[j - 1] > nb - 5) m -= 2;
				if (m > 0) {
					m = b[0];
					for (i = 2; i < j; i += 2)
						if (b[i] - b[i - 1] > m) m = b[i] - b[i - 1], k = i;
					if (nb - b[i - 1] > m) {
						m = nb - b[i - 1];
						lo = b[i - 1], hi = nb;
					} else if (b[k + 1] > nb - 5) {
						lo = b[k - 1], hi = nb;
					} else if (k == 0 || b[k - 2] < 5) {
						lo = 0, hi = b[k];
					} else {
						lo = b[k - 1], hi = b[k];
					}
					lo = lo > 5 ? (lo - 5) << kBinShift : 0;
					hi = (hi + 5) << kBinShift;
					if (m > (min_seed_len >> kBinShift) * 2 / 3) {
						chimera = 0;
						for (uint32_t q = 1; q < n_kept; ++q) {
							const OvlRec o = cand[K[q]];
							if (o.qs < (uint32_t)lo || o.qe > (uint32_t)hi) K[q] |= kDropped;
						}
					} else chimera = 1;
				} else lo = hi = 0;
			}
		}
		if (qcov > qlen * 20u && !chimera && contained < 2) {
			// hot break ends: alignment ends piling up well inside the read (128-base bins)
			const int sh = kBinShift + 1;
			for (int i = 0; i < nb / 2 + 1; ++i) bins[i] = 0;
			int s0 = nb, e0 = 0, c = 0, t = 0;
			for (uint32_t q = 1; q < n_kept; ++q) {
				if (K[q] & kDropped) continue;
				const OvlRec o = cand[K[q]];
				++c;
				int x = (int)((o.qs + 10) >> sh);
				if (x < s0) s0 = x;
				bins[x]++;
				x = (int)((o.qe - 10) >> sh);
				if (x > e0) e0 = x;
				bins[x]++;
			}
			if (c > 20) {
				while (s0 < e0 && bins[s0] < 4) ++s0;
				while (e0 > s0 && bins[e0] < 4) --e0;
				int m = 0, ms = bins[s0], me = bins[e0];
				for (int i = s0; i < e0 + 1; ++i) {
					if (i < s0 + 5 && bins[i] > ms) ms = bins[i];
					if (i > e0 - 5 && bins[i] > me) me = bins[i];
					if (bins[i] > bins[m]) m = i;
				}
				if (m > s0 + 5 && m < e0 - 5 && (float)bins[m] > 1.f * (float)(ms > me ? ms : me) && ((c > 75 && m > c / 5) || (c < 75 && m > c / 2)))
					t = m << sh;
			}
			chimera = (uint32_t)t;
			if (!hi) hi = (int)qlen;
			if (chimera <= (uint32_t)(lo + (15 << kBinShift)) || chimera + (15u << kBinShift) >= (uint32_t)hi) chimera = 0;
		}
		// survivors, in order; the self record first
		uint32_t n = 0, cont = 0;
		for (uint32_t q = 0; q < n_kept; ++q) {
			const uint32_t e = K[q];
			OvlRec o;
			if (e == kSelf) {
				o.rev = 0, o.qname = o.tname = seed, o.qs = o.ts = 0, o.qe = o.te = qlen - 1, o.match = 0;
				if (!o.qe) continue;
			} else {
				if (e & kDropped) continue;
				o = cand[e];
			}
			O[n++] = o;
			if (o.qname != o.tname && o.qs <= (uint32_t)flank && o.qe + (uint32_t)flank >= qlen) ++cont;
		}
		n_out[sd] = n;
		bl_id[sd] = seed;
		bl_kind[sd] = cont >= 2 ? (uint8_t)'c' : chimera ? (uint8_t)'k' : (uint8_t)0;
	}
}

// S3 for `ovl_sort -H` (high-quality reads): encode_ovl_filter_hq (ovl_sort.c:616-655), del_repeat_alns (:389-431),
// check_chimer_hq (:287-314) and the -H branches of ovl_filter (:433-571).  Every candidate is collected (up to the caps)
// while the two halves of bins[] count alignment starts / ends per 128 bases; overlaps that start and end at hot break
// points are repeat-induced and dropped, the 64-base coverage is rebuilt over the rest (spans that would sit above
// 2 x max_bin_cov everywhere are dropped), a bin covered at most once that no overlap spans with 15 bins to spare marks a
// chimera, and the low-coverage trimming of the raw-read path follows.  The chain is sequential per seed (lane 0 walks it;
// seeds are independent wavefronts).
__global__ void __launch_bounds__(64) seed_filter_hq_kernel(const OvlRec *__restrict__ cand, const uint32_t *__restrict__ perm,
                                                             const uint64_t *__restrict__ seed_start, uint32_t n_seeds, uint64_t n_cand,
                                                             const uint32_t *__restrict__ seed_len, int max_bin_cov, int flank, int min_seed_len,
                                                             uint32_t max_bins, uint32_t *__restrict__ kept, OvlRec *__restrict__ out,
                                                             uint32_t *__restrict__ n_out, uint32_t *__restrict__ bl_id, uint8_t *__restrict__ bl_kind)
{
	extern __shared__ uint16_t bins[];
	const uint32_t sd = blockIdx.x;
	if (sd >= n_seeds) return;
	const int lane = threadIdx.x;
	const uint64_t c0 = seed_start[sd], c1 = sd + 1 < n_seeds ? seed_start[sd + 1] : n_cand;
	const uint32_t seed = cand[perm[c0]].qname;
	const uint32_t qlen = seed_len[seed];
	const int nb = (int)(qlen >> kBinShift) + 2;
	uint32_t *K = kept + c0 + sd;
	OvlRec *O = out + c0 + sd;
	for (int i = lane; i < nb && i < (int)max_bins; i += 64) bins[i] = 0;
	__syncthreads();
	if (lane != 0) return;

	// collection + break-point histogram
	const int sh2 = kBinShift + 1;
	const int off = 1 + (int)(qlen >> sh2);
	const uint32_t qcap = qlen * 150u * 6u;
	uint32_t n_kept = 1, qcov = qlen;
	K[0] = kSelf;
	for (uint64_t c = c0; c < c1; ++c) {
		const uint32_t ci = perm[c];
		const OvlRec o = cand[ci];
		if (qcov > qcap || n_kept > 65535u - 1000u) continue;
		bins[(o.qs + 10) >> sh2]++;
		bins[((o.qe - 10) >> sh2) + off]++;
		qcov += o.qe - o.qs + 1;
		K[n_kept++] = ci;
	}
	// repeat-induced overlaps
	{
		const uint32_t fl = flank > 100 ? (uint32_t)flank * 3u : 300u;
		for (uint32_t q = 1; q < n_kept; ++q) {
			const OvlRec o = cand[K[q]];
			if (o.qs <= fl && o.qe + fl >= qlen) continue;
			if (bins[(o.qs + 10) >> sh2] >= 5 && bins[((o.qe - 10) >> sh2) + off] >= 5) K[q] |= kDropped;
		}
		for (int i = 0; i < nb; ++i) bins[i] = 0;
		for (uint32_t q = 1; q < n_kept; ++q) {
			if (K[q] & kDropped) continue;
			const OvlRec o = cand[K[q]];
			const int j = (int)((o.qs + 10) >> kBinShift), k = (int)((o.qe - 10) >> kBinShift);
			int lowest = 65535;
			for (int t = j + 1; t <= k; ++t) {
				int v = (int)bins[t] + 1;
				if (v > 65535 - 1000) --v;
				bins[t] = (uint16_t)v;
				if (v < lowest) lowest = v;
			}
			if (lowest > 2 * max_bin_cov) {
				for (int t = j + 1; t <= k; ++t) bins[t]--;
				K[q] |= kDropped;
			}
		}
	}
	// chimera: an uncovered bin inside the covered part that no overlap spans
	uint32_t chimera = 0;
	{
		int l = 0, r = nb;
		while (l < nb && bins[l] < 2) ++l;
		while (r > 0 && bins[r - 1] < 2) --r;
		for (int i = l + 1; i < r - 1 && !chimera; ++i) {
			if (bins[i] > 1) continue;
			const uint32_t lo2 = (uint32_t)(i > l + 15 ? (i - 15) << kBinShift : l << kBinShift);
			const uint32_t hi2 = (uint32_t)(i + 15 < r ? (i + 15) << kBinShift : r << kBinShift);
			bool spanned = false;
			for (uint32_t q = 1; q < n_kept && !spanned; ++q) {
				if (K[q] & kDropped) continue;
				const OvlRec o = cand[K[q]];
				spanned = o.qs < lo2 && o.qe > hi2;
			}
			if (!spanned) chimera = (uint32_t)i;
		}
	}
	int lo = 0, hi = 0;
	if (chimera) {
		int j = 0;
		uint16_t *b = bins; // (first, last) pairs of low-coverage bin runs overwrite the front of bins[]
		if (qcov > qlen * 10u) {
			const int low = 4 > max_bin_cov / 10 ? max_bin_cov / 10 : 4;
			for (int i = 1; i < nb - 1; ++i) {
				if (b[i] < low) {
					if (lo == 0) lo = i;
					hi = i;
				} else if (lo) {
					if (chimera && chimera < (uint32_t)lo && ((!j) || chimera > b[j - 1])) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
					b[j++] = (uint16_t)lo, b[j++] = (uint16_t)hi;
					lo = hi = 0;
				}
			}
			if (lo) {
				if (chimera && chimera < (uint32_t)lo && ((!j) || chimera > b[j - 1])) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
				b[j++] = (uint16_t)lo, b[j++] = (uint16_t)hi;
			}
			if (chimera && (j == 0 || chimera > b[j - 1])) b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
		} else b[j++] = (uint16_t)chimera, b[j++] = (uint16_t)chimera;
		if (j) {
			int m = j, k = 0, i;
			if (b[0] < 5) m -= 2;
			if (b[j - 1] > nb - 5) m -= 2;
			if (m > 0) {
				m = b[0];
				for (i = 2; i < j; i += 2)
					if (b[i] - b[i - 1] > m) m = b[i] - b[i - 1], k = i;
				if (nb - b[i - 1] > m) {
					m = nb - b[i - 1];
					lo = b[i - 1], hi = nb;
				} else if (b[k + 1] > nb - 5) {
					lo = b[k - 1], hi = nb;
				} else if (k == 0 || b[k - 2] < 5) {
					lo = 0, hi = b[k];
				} else {
					lo = b[k - 1], hi = b[k];
				}
				lo = lo > 5 ? (lo - 5) << kBinShift : 0;
				hi = (hi + 5) << kBinShift;
				if (m > (min_seed_len >> kBinShift) * 2 / 3) {
					chimera = 0;
					for (uint32_t q = 1; q < n_kept; ++q) {
						if (K[q] & kDropped) continue;
						const OvlRec o = cand[K[q]];
						if (o.qs < (uint32_t)lo || o.qe > (uint32_t)hi) K[q] |= kDropped;
					}
				} else chimera = 1;
			}
		}
	}
	// survivors, in order; the self record first.  A containing overlap of high-quality reads must be >= 90 % matches.
	uint32_t n = 0, cont = 0;
	for (uint32_t q = 0; q < n_kept; ++q) {
		const uint32_t e = K[q];
		OvlRec o;
		if (e == kSelf) {
			o.rev = 0, o.qname = o.tname = seed, o.qs = o.ts = 0, o.qe = o.te = qlen - 1, o.match = 0;
			if (!o.qe) continue;
		} else {
			if (e & kDropped) continue;
			o = cand[e];
		}
		O[n++] = o;
		if (o.qname != o.tname && o.qs <= (uint32_t)flank && o.qe + (uint32_t)flank >= qlen && (double)o.match >= (double)(o.qe - o.qs + 1) * 0.9) ++cont;
	}
	n_out[sd] = n;
	bl_id[sd] = seed;
	bl_kind[sd] = cont >= 2 ? (uint8_t)'c' : chimera ? (uint8_t)'k' : (uint8_t)0;
}

void launch_seed_filter(const OvlRec *cand, const uint32_t *perm, const uint64_t *seed_start, uint32_t n_seeds, uint64_t n_cand,
                        const uint32_t *seed_len, int max_bin_cov, int flank, int min_seed_len, uint32_t max_bins, uint32_t *kept, OvlRec *out,
                        uint32_t *n_out, uint32_t *bl_id, uint8_t *bl_kind, bool hq, hipStream_t s)
{
	if (n_seeds && hq) ND_LAUNCH(seed_filter_hq_kernel, dim3(n_seeds), dim3(64), (size_t)max_bins * 2, s, cand, perm, seed_start, n_seeds,
	                                      n_cand, seed_len, max_bin_cov, flank, min_seed_len, max_bins, kept, out, n_out, bl_id, bl_kind);
	else if (n_seeds) ND_LAUNCH(seed_filter_kernel, dim3(n_seeds), dim3(64), (size_t)max_bins * 2, s, cand, perm, seed_start, n_seeds, n_cand,
	                                seed_len, max_bin_cov, flank, min_seed_len, max_bins, kept, out, n_out, bl_id, bl_kind);
}

// dense output: seed sd's records start at out + seed_start[sd] + sd
__global__ void compact_seed_recs_kernel(const uint64_t *__restrict__ seed_start, uint32_t n_seeds, const OvlRec *__restrict__ out,
                                         const uint32_t *__restrict__ n_out, const uint64_t *__restrict__ off, OvlRec *__restrict__ dense)
{
	const uint32_t sd = blockIdx.x;
	if (sd >= n_seeds) return;
	const OvlRec *src = out + seed_start[sd] + sd;
	OvlRec *dst = dense + off[sd];
	for (uint32_t i = threadIdx.x; i < n_out[sd]; i += blockDim.x) dst[i] = src[i];
}

void launch_compact_seed_recs(const uint64_t *seed_start, uint32_t n_seeds, const OvlRec *out, const uint32_t *n_out, const uint64_t *off,
                              OvlRec *dense, hipStream_t s)
{
	if (n_seeds) ND_LAUNCH(compact_seed_recs_kernel, dim3(n_seeds), dim3(64), 0, s, seed_start, n_seeds, out, n_out, off, dense);
}

// ------------------------------------------------------------------------------------------------
// K16: pile admission (read_seq_data, lib/nextcorrect.py:92-143) on the dense sorted records, one wavefront per group (a run of
// records with one seed id in field 0; group g = recs[off[g] .. off[g + 1])).  The reference loop carries state from record to
// record; on a well-formed stream that state is, per group, one prefix sum:
//   seed_len = t_e + 1 of the group's first record; the seed is valid iff seed_len >= min_len_seed and it is not in the skip set;
//   a record is a candidate iff t_e - t_s >= min_len_aln; only the first candidate of a query read counts; `before` = the spans
//   (t_e - t_s + 1) of the counting records in front of it; it is admitted iff !(before / seed_len > 1.5 * max_cov_aln);
//   the pile is kept iff total / seed_len >= min_cov_seed.
// `before` only grows, so the first counting record that fails the depth test ends the group (in the loop nothing is admitted and
// nothing marked behind it, so "counting" and "admitted" are the same records in front of it).
// The two comparisons are the host's own: both sums converted to double (round to nearest, as on the host), one IEEE division
// (correctly rounded in device code built without fast-math), compared with a limit that is exact in a double (1.5 x a 32-bit
// integer).  Operation for operation ndgpu_assemble_piles's arithmetic, so the verdicts are equal for every total, with no
// 64-bit product (3 * max_cov_aln * seed_len does not fit 64 bits when both are large) and no bound on the totals to argue.
// Where the loop's last_seed / '+' state would split a group again -- a valid seed whose first record is not admitted, a rejected seed
// one of whose later records passes as a seed, t_e < t_s, a query id >= n_ids (the host does not de-duplicate those) -- the group is
// irregular: lane 0 counts it in counters[0] (one atomic per such group; any non-zero value is the flag) and the host side
// answers the whole call with ndgpu_assemble_piles.
// The query reads seen so far are an open-addressing table of 64-bit slots, (query id + 1) << 32 | number of the record in its
// group, 0 = empty: a slot is claimed with a compare-and-swap and lowered with an atomic minimum, so the first occurrence owns it
// whatever order lanes and probes run in; a chunk of 64 records inserts, then every lane reads its slot back.  Groups of up to
// half of kAdmitLdsSlots records (or of the forced capacity, NDGPU_ADMIT_TABLE) keep the table in LDS, larger ones ("wide") in
// their slice of a global scratch region, pow2ceil(2 x records) slots: never more than half full either way.

constexpr uint32_t kAdmitLdsSlots = 2048;   // 16 KB of LDS: groups of up to 1024 records
constexpr uint32_t kNoSlot = 0xffffffffu;

__device__ __forceinline__ uint32_t pow2ceil_u32(uint32_t v) { uint32_t p = 2; while (p < v) p <<= 1; return p; }

__global__ void group_flag_kernel(const OvlRec *__restrict__ recs, uint64_t n, uint32_t *__restrict__ flag)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) flag[i] = i == 0 || recs[i].qname != recs[i - 1].qname;
}

// skip set as a bitmap over the read ids: ids[i] joins when kind == nullptr (the caller's list) or kind[i] != 0 (a `.bl` verdict)
__global__ void skip_bits_kernel(const uint32_t *__restrict__ ids, const uint8_t *__restrict__ kind, uint64_t n, uint32_t n_ids,
                                 uint32_t *__restrict__ bits)
{
	uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n || (kind && !kind[i])) return;
	const uint32_t id = ids[i];
	if (id < n_ids) atomicOr(bits + (id >> 5), 1u << (id & 31));
}

// slots of the global table of every group that does not fit the LDS one (0: it does); counters[1] = such groups
__global__ void admit_plan_kernel(const uint64_t *__restrict__ off, uint32_t n_groups, uint32_t lds_slots, uint32_t *__restrict__ slots,
                                  uint32_t *__restrict__ counters)
{
	uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
	if (g >= n_groups) return;
	const uint64_t cnt = off[g + 1] - off[g];   // (< 2^30: the host side refuses longer streams)
	const bool wide = 2 * cnt > lds_slots;
	slots[g] = wide ? pow2ceil_u32((uint32_t)(2 * cnt)) : 0;
	if (wide) atomicAdd(counters + 1, 1u);
}

// the slot that record `idx` of the group holds for query read q, or kNoSlot when an earlier record already holds it
__device__ __forceinline__ uint32_t seen_insert(unsigned long long *tab, uint32_t mask, uint32_t shift, uint32_t q, uint32_t idx)
{
	const unsigned long long mine = ((unsigned long long)q + 1) << 32 | idx;
	uint32_t h = (q * 2654435761u) >> shift;
	for (;;) {
		const unsigned long long old = atomicCAS(tab + h, 0ull, mine);
		if (old == 0) return h;
		if ((old >> 32) == (mine >> 32)) return atomicMin(tab + h, mine) < mine ? kNoSlot : h;   // (the value found decides: the atomic has finished)
		h = (h + 1) & mask;
	}
}

__device__ __forceinline__ unsigned long long wave_excl_sum_u64(unsigned long long v, int lane, unsigned long long *total)
{
	unsigned long long s = v;
	for (int d = 1; d < 64; d <<= 1) {
		const unsigned long long o = __shfl_up(s, d, 64);
		if (lane >= d) s += o;
	}
	*total = __shfl(s, 63, 64);
	return s - v;
}

struct AdmitArgs {
	const OvlRec *recs;
	const uint64_t *off;
	const uint32_t *skip_bits;
	uint32_t n_groups, n_ids, min_len_seed, min_len_aln, max_cov_aln, min_cov_seed;
	uint8_t *adm;         // per record: admitted (zeroed by the caller)
	uint32_t *n_adm;      // per group: records of its pile (0: no pile)
	uint32_t *kept;       // per group: 1 = a pile
	uint32_t *counters;   // [0] irregular groups
};

// tab: `slots` zeroed-by-us slots of this group (a power of two >= 2 x its records); global: tab is device memory
__device__ __forceinline__ void admit_group(const AdmitArgs &A, uint32_t g, unsigned long long *tab, uint32_t slots, bool global)
{
	const int lane = threadIdx.x;
	const uint64_t c0 = A.off[g], c1 = A.off[g + 1];
	if (c0 == c1) return;   // (a seed the sort left nothing of: n_adm / kept stay 0)
	const OvlRec first = A.recs[c0];
	const uint32_t seed = first.qname;
	const unsigned long long seed_len = (unsigned long long)first.qe + 1;
	const bool skipped = seed < A.n_ids && (A.skip_bits[seed >> 5] >> (seed & 31) & 1);
	const bool valid = seed_len >= A.min_len_seed && !skipped;
	bool irregular = valid && first.qe - first.qs < A.min_len_aln;
	const uint32_t mask = slots - 1, shift = 32 - (uint32_t)(__ffs((int)slots) - 1);
	if (valid) {
		for (uint32_t i = lane; i < slots; i += 64) tab[i] = 0;
		if (global) __threadfence();   // the zeroes are in place before another lane's atomic finds the slot
		ND_LOCKSTEP();
	}
	const double lim = (double)A.max_cov_aln * 1.5;
	unsigned long long before = 0;
	uint32_t n = 0;
	for (uint64_t base = c0; base < c1; base += 64) {
		const uint64_t k = base + lane;
		const bool live = k < c1;
		OvlRec r = first;
		if (live) r = A.recs[k];
		bool bad = live && (r.qe < r.qs || r.tname >= A.n_ids);
		if (!valid) bad = bad || (live && !skipped && (unsigned long long)r.qe + 1 >= A.min_len_seed);   // the loop would start a pile here
		if (__ballot(bad)) irregular = true;
		if (!valid) continue;
		if (irregular) break;
		const uint32_t idx = (uint32_t)(k - c0);
		uint32_t slot = kNoSlot;
		if (live && r.qe - r.qs >= A.min_len_aln) slot = seen_insert(tab, mask, shift, r.tname, idx);
		ND_LOCKSTEP();   // every insert of the chunk before any read-back
		bool counting = false;
		if (slot != kNoSlot) counting = (uint32_t)__hip_atomic_load(tab + slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == idx;
		const unsigned long long span = counting ? (unsigned long long)(r.qe - r.qs) + 1 : 0;
		unsigned long long chunk_total;
		const unsigned long long mine_before = before + wave_excl_sum_u64(span, lane, &chunk_total);
		const bool admitted = counting && !((double)mine_before / (double)seed_len > lim);
		const unsigned long long am = __ballot(admitted), fm = __ballot(counting && !admitted);
		if (admitted) A.adm[k] = 1;
		n += (uint32_t)__popcll(am);
		if (fm) {   // the depth limit: nothing behind this record is admitted
			before = __shfl(mine_before, __ffsll((long long)fm) - 1, 64);
			break;
		}
		before += chunk_total;
	}
	if (lane == 0) {
		const bool keep = valid && !irregular && (double)before / (double)seed_len >= (double)A.min_cov_seed;
		A.n_adm[g] = keep ? n : 0;
		A.kept[g] = keep;
		if (irregular) atomicAdd(A.counters, 1u);
	}
}

__global__ void __launch_bounds__(64) admit_count_kernel(AdmitArgs A, uint32_t lds_slots, const uint32_t *__restrict__ wide_slots,
                                                          const uint64_t *__restrict__ tab_off, unsigned long long *__restrict__ scratch)
{
	__shared__ unsigned long long lds_tab[kAdmitLdsSlots];
	const uint32_t g = blockIdx.x;
	if (g >= A.n_groups) return;
	const uint32_t ws = wide_slots[g];
	if (ws) {
		admit_group(A, g, scratch + tab_off[g], ws, true);
	} else {
		const uint64_t cnt = A.off[g + 1] - A.off[g];   // 2 * cnt <= lds_slots <= kAdmitLdsSlots (admit_plan_kernel)
		admit_group(A, g, lds_tab, pow2ceil_u32((uint32_t)(2 * cnt)), false);
	}
}

// second pass: the admitted records of every kept group as rows (seed, rev, seed start, seed end, read, read start, read end,
// match) from rec_off[g] on, and the pile's entry
__global__ void __launch_bounds__(64) admit_emit_kernel(const OvlRec *__restrict__ recs, const uint64_t *__restrict__ off, uint32_t n_groups,
                                                         const uint8_t *__restrict__ adm, const uint32_t *__restrict__ n_adm,
                                                         const uint32_t *__restrict__ kept, const uint64_t *__restrict__ rec_off,
                                                         const uint64_t *__restrict__ pile_idx, uint32_t *__restrict__ recs8,
                                                         uint64_t *__restrict__ pile_off, uint32_t *__restrict__ seeds)
{
	const uint32_t g = blockIdx.x;
	if (g >= n_groups || !kept[g]) return;
	const int lane = threadIdx.x;
	const uint64_t c0 = off[g], c1 = off[g + 1], o = rec_off[g];
	const uint32_t want = n_adm[g];
	if (lane == 0) pile_off[pile_idx[g]] = o, seeds[pile_idx[g]] = recs[c0].qname;
	uint32_t done = 0;
	for (uint64_t base = c0; base < c1 && done < want; base += 64) {
		const uint64_t k = base + lane;
		const bool a = k < c1 && adm[k];
		const unsigned long long m = __ballot(a);
		if (a) {
			const OvlRec r = recs[k];
			uint32_t *row = recs8 + (o + done + (uint32_t)__popcll(m & ((1ull << lane) - 1))) * 8;
			row[0] = r.qname, row[1] = r.rev, row[2] = r.qs, row[3] = r.qe, row[4] = r.tname, row[5] = r.ts, row[6] = r.te, row[7] = r.match;
		}
		done += (uint32_t)__popcll(m);
	}
}

void launch_group_flag(const OvlRec *recs, uint64_t n, uint32_t *flag, hipStream_t s)
{
	if (n) ND_LAUNCH(group_flag_kernel, GRID1(n), 0, s, recs, n, flag);
}
void launch_skip_bits(const uint32_t *ids, const uint8_t *kind, uint64_t n, uint32_t n_ids, uint32_t *bits, hipStream_t s)
{
	if (n) ND_LAUNCH(skip_bits_kernel, GRID1(n), 0, s, ids, kind, n, n_ids, bits);
}
uint32_t admit_lds_slots() { return kAdmitLdsSlots; }
void launch_admit_plan(const uint64_t *off, uint32_t n_groups, uint32_t lds_slots, uint32_t *slots, uint32_t *counters, hipStream_t s)
{
	if (n_groups) ND_LAUNCH(admit_plan_kernel, GRID1(n_groups), 0, s, off, n_groups, lds_slots, slots, counters);
}
void launch_admit_count(const OvlRec *recs, const uint64_t *off, uint32_t n_groups, const uint32_t *skip_bits, uint32_t n_ids,
                        uint32_t min_len_seed, uint32_t min_len_aln, uint32_t max_cov_aln, uint32_t min_cov_seed, uint32_t lds_slots,
                        const uint32_t *wide_slots, const uint64_t *tab_off, uint64_t *scratch, uint8_t *adm, uint32_t *n_adm, uint32_t *kept,
                        uint32_t *counters, hipStream_t s)
{
	AdmitArgs A;
	A.recs = recs, A.off = off, A.skip_bits = skip_bits, A.n_groups = n_groups, A.n_ids = n_ids, A.min_len_seed = min_len_seed;
	A.min_len_aln = min_len_aln, A.max_cov_aln = max_cov_aln, A.min_cov_seed = min_cov_seed, A.adm = adm, A.n_adm = n_adm, A.kept = kept;
	A.counters = counters;
	if (n_groups) ND_LAUNCH(admit_count_kernel, dim3(n_groups), dim3(64), 0, s, A, lds_slots, wide_slots, tab_off, (unsigned long long*)scratch);
}
void launch_admit_emit(const OvlRec *recs, const uint64_t *off, uint32_t n_groups, const uint8_t *adm, const uint32_t *n_adm,
                       const uint32_t *kept, const uint64_t *rec_off, const uint64_t *pile_idx, uint32_t *recs8, uint64_t *pile_off,
                       uint32_t *seeds, hipStream_t s)
{
	if (n_groups) ND_LAUNCH(admit_emit_kernel, dim3(n_groups), dim3(64), 0, s, recs, off, n_groups, adm, n_adm, kept, rec_off, pile_idx, recs8,
	                        pile_off, seeds);
}

// ------------------------------------------------------------------------------------------------
// K17: the `.ovl` codec (encode_ovl / decode_ovl, lib/ovl.c:105-203; the host loops are ndgpu_ovl_encode / ndgpu_ovl_decode).
// A record is 8 big-endian base-128 varints (a byte < 128 ends a value), the two read names delta-coded against the record in front.
//
// Decode.  The images of a call's files lie in one device buffer, every file at a multiple of kCodecTile bytes; a tile (one wavefront,
// kCodecIters x 64 lanes x 16 bytes) belongs to one file.  The host loop's value is v = (v << 7) | (c & 127) in uint32_t over the
// bytes since the last terminator: whatever lies more than 4 bytes in front of the terminator has been shifted out of the 32 bits,
// and the 5th-from-last byte keeps its low 4 bits.  So a value is a function of its terminator and of at most the 4 bytes in front of
// it, for EVERY byte string -- over-long values, runs of continuation bytes, anything -- and every terminator is found by looking at
// its own byte alone.  That is why this path has no "malformed input" decline: there is no input on which it differs from the loop.
// Value j of a file is field j % 8 of record j / 8 (a file's values beyond its last whole record are dropped), and j is a prefix
// count of terminators: per lane a popcount, per wavefront a prefix, per tile a total the host side scans.
// The names are running sums of +-delta in wrapping 32-bit arithmetic: addition modulo 2^32 is associative, so an exclusive scan of
// the two's-complement deltas (summed in 64 bits, truncated) is the loop's `prev`; a file's own sum starts at its first record.
//
// Encode.  One lane per record; the predecessor's names come from the lane below.  Sizes, a scan, then each wavefront stages the
// bytes of its 64 records in LDS at the alignment they have in the output and stores the span with dword stores (byte stores for
// the up to 3 bytes in front of the first and behind the last whole dword): every output byte has one writer, no atomics.

constexpr uint32_t kCodecIters = 4;
constexpr uint32_t kCodecTile = kCodecIters * 64 * 16;   // bytes of a decode tile

// what a decode launch knows of the files: file f = img[start[f] .. start[f] + bytes[f]), its tiles tile0[f] .. tile0[f + 1]
struct CodecFiles {
	const uint8_t *img;
	const uint64_t *start, *bytes, *tile0;
	const uint32_t *tile_file;
};

// the 16-bit terminator mask of 16 bytes (bit i: byte i < 128), the first `valid` bytes of them
__device__ __forceinline__ uint32_t term_mask16(const uint4 w, uint32_t valid)
{
	// per word: bit 0, 8, 16, 24 = the byte is a terminator; the multiply gathers them into bits 24..27 (all partial products land on
	// distinct bits, so there is no carry)
	const uint32_t a = ((~w.x >> 7 & 0x01010101u) * 0x01020408u) >> 24 & 15u, b = ((~w.y >> 7 & 0x01010101u) * 0x01020408u) >> 24 & 15u;
	const uint32_t c = ((~w.z >> 7 & 0x01010101u) * 0x01020408u) >> 24 & 15u, d = ((~w.w >> 7 & 0x01010101u) * 0x01020408u) >> 24 & 15u;
	const uint32_t m = a | b << 4 | c << 8 | d << 12;
	return valid >= 16 ? m : m & ((1u << valid) - 1u);
}

__device__ __forceinline__ uint32_t wave_incl_sum_u32(uint32_t v, int lane)
{
	for (int d = 1; d < 64; d <<= 1) {
		const uint32_t o = __shfl_up(v, d, 64);
		if (lane >= d) v += o;
	}
	return v;
}

// the lane's 16 bytes of iteration `it` of tile `t` (file-relative offset *at), and how many of them are the file's
__device__ __forceinline__ uint4 codec_load(const CodecFiles &F, uint32_t f, uint64_t t, uint32_t it, int lane, uint64_t *at, uint32_t *valid)
{
	const uint64_t o = (t - F.tile0[f]) * kCodecTile + (uint64_t)it * 1024 + (uint64_t)lane * 16, nb = F.bytes[f];
	*at = o;
	*valid = o >= nb ? 0u : (nb - o >= 16 ? 16u : (uint32_t)(nb - o));
	// (the buffer is whole tiles: the load is inside it wherever the file ends; start[f] is a multiple of the tile)
	return *reinterpret_cast<const uint4*>(F.img + F.start[f] + o);
}

__global__ void __launch_bounds__(64) codec_count_kernel(CodecFiles F, uint64_t n_tiles, uint32_t *__restrict__ tile_cnt)
{
	const uint64_t t = blockIdx.x;
	if (t >= n_tiles) return;
	const int lane = threadIdx.x;
	const uint32_t f = F.tile_file[t];
	uint32_t cnt = 0;
	for (uint32_t it = 0; it < kCodecIters; ++it) {
		uint64_t at;
		uint32_t valid;
		const uint4 w = codec_load(F, f, t, it, lane, &at, &valid);
		cnt += (uint32_t)__popc(term_mask16(w, valid));
	}
	cnt = wave_incl_sum_u32(cnt, lane);
	if (lane == 63) tile_cnt[t] = cnt;
}

// whole records of every file (tile_first = the exclusive scan of tile_cnt, n_tiles + 1 entries)
__global__ void codec_file_plan_kernel(const uint64_t *__restrict__ tile0, const uint64_t *__restrict__ tile_first, uint32_t n_files,
                                       uint64_t *__restrict__ n_rec)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f < n_files) n_rec[f] = (tile_first[tile0[f + 1]] - tile_first[tile0[f]]) >> 3;
}

// fields[8 * (rec_base[f] + j / 8) + j % 8] = value j of file f; consumed[f] = the offset behind the last byte of its last whole
// record (zeroed by the caller: a file without a whole record consumes nothing)
__global__ void __launch_bounds__(64) codec_emit_kernel(CodecFiles F, uint64_t n_tiles, const uint64_t *__restrict__ tile_first,
                                                         const uint64_t *__restrict__ n_rec, const uint64_t *__restrict__ rec_base,
                                                         uint32_t *__restrict__ fields, uint64_t *__restrict__ consumed)
{
	const uint64_t t = blockIdx.x;
	if (t >= n_tiles) return;
	const int lane = threadIdx.x;
	const uint32_t f = F.tile_file[t];
	const uint64_t want = n_rec[f] * 8;                               // values of the file that belong to whole records
	uint64_t j0 = tile_first[t] - tile_first[F.tile0[f]];             // file-relative index of the tile's first value
	if (j0 >= want) return;                                           // (the whole wavefront: nothing but the partial tail)
	uint32_t *const out = fields + rec_base[f] * 8;
	const uint8_t *const file = F.img + F.start[f];
	for (uint32_t it = 0; it < kCodecIters; ++it) {
		uint64_t at;
		uint32_t valid;
		const uint4 w = codec_load(F, f, t, it, lane, &at, &valid);
		uint32_t m = term_mask16(w, valid);
		const uint32_t mine = (uint32_t)__popc(m), incl = wave_incl_sum_u32(mine, lane);
		uint64_t j = j0 + (incl - mine);
		j0 += __shfl(incl, 63, 64);
		const unsigned long long lo = (unsigned long long)w.y << 32 | w.x, hi = (unsigned long long)w.w << 32 | w.z;
		while (m) {
			const int i = __ffs((int)m) - 1;
			m &= m - 1;
			if (j >= want) break;
			uint32_t v = (uint32_t)((i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8))) & 0xffu);
			const uint64_t p = at + (uint32_t)i;                      // the terminator's offset in the file
#pragma unroll
			for (int k = 1; k <= 4; ++k) {
				if (p < (uint64_t)k) break;                            // the start of the file: nothing in front
				const int q = i - k;
				// in front of the lane's 16 bytes (another lane's, another iteration's, another tile's): a plain load
				const uint32_t b = q >= 0 ? (uint32_t)((q < 8 ? lo >> (8 * q) : hi >> (8 * (q - 8))) & 0xffu) : (uint32_t)file[p - k];
				if (b < 128) break;
				v |= (b & 127u) << (7 * k);                            // (k = 4: the low 4 bits stay, as in the loop's uint32_t)
			}
			out[j] = v;
			if (j + 1 == want) consumed[f] = p + 1;
			++j;
		}
	}
}

__device__ __forceinline__ uint32_t file_of_record(const uint64_t *__restrict__ rec_base, uint32_t n_files, uint64_t i)
{
	uint32_t lo = 0, hi = n_files;   // the last f with rec_base[f] <= i (files without records share their successor's base)
	while (hi - lo > 1) {
		const uint32_t mid = lo + (hi - lo) / 2;
		if (rec_base[mid] <= i) lo = mid; else hi = mid;
	}
	return lo;
}

// the signed name deltas of every record as 32-bit two's complement (fields as codec_emit_kernel left them)
__global__ void codec_delta_kernel(const uint32_t *__restrict__ fields, uint64_t n, uint32_t *__restrict__ dq, uint32_t *__restrict__ dt)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t *f = fields + i * 8;
	const uint32_t fl = f[1];
	dq[i] = (fl & 2) ? 0u - f[0] : f[0];
	dt[i] = (fl & 4) ? 0u - f[4] : f[4];
}

// fields -> records, in place (a lane reads its own 8 words, then writes them); sq / st = exclusive scans of dq / dt
__global__ void codec_records_kernel(uint32_t *__restrict__ fields, uint64_t n, const uint32_t *__restrict__ dq, const uint32_t *__restrict__ dt,
                                     const uint64_t *__restrict__ sq, const uint64_t *__restrict__ st, const uint64_t *__restrict__ rec_base,
                                     uint32_t n_files)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	uint32_t *const p = fields + i * 8;
	const uint4 a = *reinterpret_cast<const uint4*>(p), b = *reinterpret_cast<const uint4*>(p + 4);   // f0..f3, f4..f7
	const uint64_t r0 = rec_base[file_of_record(rec_base, n_files, i)];   // the file restarts from prev = {0, 0}
	const uint32_t fl = a.y;
	OvlRec r;
	r.rev = fl & 1;
	r.qname = (uint32_t)(sq[i] - sq[r0]) + dq[i];
	r.qs = a.z;
	r.qe = a.z + a.w;
	r.tname = (uint32_t)(st[i] - st[r0]) + dt[i];
	r.ts = b.y;
	r.te = (fl & 8) ? b.y + a.w + b.z : b.y + a.w - b.z;
	r.match = b.w;
	*reinterpret_cast<uint4*>(p) = make_uint4(r.rev, r.qname, r.qs, r.qe);
	*reinterpret_cast<uint4*>(p + 4) = make_uint4(r.tname, r.ts, r.te, r.match);
}

// ---- encode
__device__ __forceinline__ uint32_t varint_len(uint32_t v) { return v < 128 ? 1u : (uint32_t)(32 - __clz((int)v) + 6) / 7u; }

// the eight fields of ndgpu_ovl_encode for record r behind a record named (pq, pt)
__device__ __forceinline__ void encode_fields(const OvlRec &r, uint32_t pq, uint32_t pt, uint32_t fld[8])
{
	uint32_t flags = r.rev;
	const uint32_t qspan = r.qe - r.qs, tspan = r.te - r.ts;
	fld[3] = qspan;
	if (r.qname >= pq) fld[0] = r.qname - pq; else flags |= 2, fld[0] = pq - r.qname;
	if (r.tname >= pt) fld[4] = r.tname - pt; else flags |= 4, fld[4] = pt - r.tname;
	if (qspan >= tspan) fld[6] = qspan - tspan; else flags |= 8, fld[6] = tspan - qspan;
	fld[1] = flags & 0xff, fld[2] = r.qs, fld[5] = r.ts, fld[7] = r.match;
}

// record i and its fields; the predecessor's names from the lane below, lane 0 reads them (record 0: the caller's prev).  Every lane of
// the wavefront calls this (the lanes behind the last record with live = false).
__device__ __forceinline__ void encode_record(const OvlRec *__restrict__ recs, uint64_t i, bool live, int lane, uint32_t prev_q, uint32_t prev_t,
                                              uint32_t fld[8])
{
	OvlRec r = {0, 0, 0, 0, 0, 0, 0, 0};
	if (live) r = recs[i];
	uint32_t pq = __shfl_up(r.qname, 1, 64), pt = __shfl_up(r.tname, 1, 64);
	if (lane == 0) {
		pq = prev_q, pt = prev_t;
		if (live && i > 0) pq = recs[i - 1].qname, pt = recs[i - 1].tname;
	}
	encode_fields(r, pq, pt, fld);
}

__global__ void __launch_bounds__(64) codec_size_kernel(const OvlRec *__restrict__ recs, uint64_t n, uint32_t prev_q, uint32_t prev_t,
                                                         uint32_t *__restrict__ len)
{
	const int lane = threadIdx.x;
	const uint64_t i = (uint64_t)blockIdx.x * 64 + lane;
	uint32_t fld[8];
	encode_record(recs, i, i < n, lane, prev_q, prev_t, fld);
	uint32_t nb = 0;
#pragma unroll
	for (int k = 0; k < 8; ++k) nb += varint_len(fld[k]);
	if (i < n) len[i] = nb;   // 8 .. 37: seven values of up to 5 bytes, the flags (masked to 8 bits) of up to 2
}

constexpr uint32_t kEncStageWords = (64 * 40 + 3 + 3) / 4 + 1;   // 64 records of 40 bytes behind up to 3 bytes of alignment

// off = the exclusive scan of len (n + 1 entries); out is 4-byte aligned
__global__ void __launch_bounds__(64) codec_write_kernel(const OvlRec *__restrict__ recs, uint64_t n, uint32_t prev_q, uint32_t prev_t,
                                                          const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
	__shared__ uint32_t stage_w[kEncStageWords];
	uint8_t *const stage = reinterpret_cast<uint8_t*>(stage_w);
	const int lane = threadIdx.x;
	const uint64_t i0 = (uint64_t)blockIdx.x * 64, i = i0 + lane;
	const uint64_t i1 = i0 + 64 < n ? i0 + 64 : n;
	const uint64_t g0 = off[i0], g1 = off[i1];
	const uint32_t head = (uint32_t)(g0 & 3);   // the stage holds the span at the alignment it has in `out`
	uint32_t fld[8];
	encode_record(recs, i, i < n, lane, prev_q, prev_t, fld);
	if (i < n) {
		uint32_t at = head + (uint32_t)(off[i] - g0);
#pragma unroll
		for (int k = 0; k < 8; ++k) {
			const uint32_t v = fld[k];
			for (int g = (int)varint_len(v) - 1; g >= 0; --g) stage[at++] = (uint8_t)((v >> (7 * g) & 127u) | (g ? 128u : 0u));
		}
	}
	__syncthreads();
	const uint32_t end = head + (uint32_t)(g1 - g0);                 // stage[head .. end) = out[g0 .. g1)
	const uint32_t w_lo = (head + 3) & ~3u, w_hi = end & ~3u;        // whole dwords: stage[w_lo .. w_hi)
	const uint32_t head_end = w_lo < end ? w_lo : end;
	uint8_t *const base = out + (g0 - head);                          // of stage[0]: a dword boundary of `out`
	if (head + lane < head_end) base[head + lane] = stage[head + lane];
	for (uint32_t x = w_lo + 4 * (uint32_t)lane; x < w_hi; x += 256) *reinterpret_cast<uint32_t*>(base + x) = stage_w[x >> 2];
	const uint32_t tail = w_hi > head_end ? w_hi : head_end;
	if (tail + lane < end) base[tail + lane] = stage[tail + lane];
}

uint32_t codec_tile_bytes() { return kCodecTile; }
void launch_codec_count(const uint8_t *img, const uint64_t *start, const uint64_t *bytes, const uint64_t *tile0, const uint32_t *tile_file,
                        uint64_t n_tiles, uint32_t *tile_cnt, hipStream_t s)
{
	const CodecFiles F{img, start, bytes, tile0, tile_file};
	if (n_tiles) ND_LAUNCH(codec_count_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, F, n_tiles, tile_cnt);
}
void launch_codec_file_plan(const uint64_t *tile0, const uint64_t *tile_first, uint32_t n_files, uint64_t *n_rec, hipStream_t s)
{
	if (n_files) ND_LAUNCH(codec_file_plan_kernel, GRID1(n_files), 0, s, tile0, tile_first, n_files, n_rec);
}
void launch_codec_emit(const uint8_t *img, const uint64_t *start, const uint64_t *bytes, const uint64_t *tile0, const uint32_t *tile_file,
                       uint64_t n_tiles, const uint64_t *tile_first, const uint64_t *n_rec, const uint64_t *rec_base, OvlRec *recs,
                       uint64_t *consumed, hipStream_t s)
{
	const CodecFiles F{img, start, bytes, tile0, tile_file};
	if (n_tiles) ND_LAUNCH(codec_emit_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, F, n_tiles, tile_first, n_rec, rec_base, (uint32_t*)recs, consumed);
}
void launch_codec_delta(const OvlRec *recs, uint64_t n, uint32_t *dq, uint32_t *dt, hipStream_t s)
{
	if (n) ND_LAUNCH(codec_delta_kernel, GRID1(n), 0, s, (const uint32_t*)recs, n, dq, dt);
}
void launch_codec_records(OvlRec *recs, uint64_t n, const uint32_t *dq, const uint32_t *dt, const uint64_t *sq, const uint64_t *st,
                          const uint64_t *rec_base, uint32_t n_files, hipStream_t s)
{
	if (n) ND_LAUNCH(codec_records_kernel, GRID1(n), 0, s, (uint32_t*)recs, n, dq, dt, sq, st, rec_base, n_files);
}
void launch_codec_size(const OvlRec *recs, uint64_t n, uint32_t prev_q, uint32_t prev_t, uint32_t *len, hipStream_t s)
{
	if (n) ND_LAUNCH(codec_size_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, recs, n, prev_q, prev_t, len);
}
void launch_codec_write(const OvlRec *recs, uint64_t n, uint32_t prev_q, uint32_t prev_t, const uint64_t *off, uint8_t *out, hipStream_t s)
{
	if (n) ND_LAUNCH(codec_write_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, recs, n, prev_q, prev_t, off, out);
}

// ------------------------------------------------------------------------------------------------
// K18: the stable split of a record set by file (ndgpu_ovl_recset_split; on the host: np.argsort(file_of[qname], kind="stable") and a
// cut at the file boundaries -- stage.Shard._overlaps_grouped).  File f's output is the records with file_of[qname] == f in input
// order, so a record's output row is
//     (records of files < f)  +  (records of file f in earlier tiles)  +  (records of file f earlier in its own tile).
// A tile is kSplitIters x 64 consecutive records and belongs to one wavefront.  The count pass leaves cnt[f][tile]; an exclusive scan
// over that table in file-major order is the first two terms for every (file, tile) at once, and its entries at the start of every
// file's row are the cut points.  The scatter pass walks its tile again in the same order and keeps the third term as a running
// count per file.  Inside a 64-record iteration the lanes of one file are told apart by ballots: the wavefront takes the file of its
// first live lane, ballots the lanes that have the same one -- the popcount of the lower lanes in that ballot is the record's rank
// among them --, drops them, and goes on until no lane is live: one round per distinct file present (mostly one or two; 64 at worst).
// The per-file counts of a wavefront live in registers: lane l holds files l, l + 64, l + 128, l + 192 (n_files <= kSplitMaxFiles),
// read by the others with a shuffle and advanced by their owner.  No LDS, no atomics on a position, nothing that depends on the order
// lanes or wavefronts run in: every output row is a function of the input alone.
// A record whose qname >= n_ids or whose file is not one of the n_files (0xffffffff = "no file") is counted in *bad and left out; the
// host side then makes no set.

constexpr uint32_t kSplitIters = 8;
constexpr uint32_t kSplitTile = kSplitIters * 64;   // records of a tile
constexpr uint32_t kSplitMaxFiles = 256;
constexpr uint32_t kSplitSlots = kSplitMaxFiles / 64;

// the file of record i (kNoSlot behind the last record), and whether the record is one the split refuses
__device__ __forceinline__ uint32_t split_file(const OvlRec *__restrict__ recs, uint64_t i, uint64_t n, const uint32_t *__restrict__ file_of,
                                               uint32_t n_ids, uint32_t n_files, bool *bad)
{
	*bad = false;
	if (i >= n) return kNoSlot;
	const uint32_t q = recs[i].qname;
	const uint32_t f = q < n_ids ? file_of[q] : kNoSlot;
	*bad = f >= n_files;
	return f;
}

// the slot of v that belongs to file f (f wave-uniform; selects, so that v stays in registers)
template <class T> __device__ __forceinline__ T split_slot(const T (&v)[kSplitSlots], uint32_t f)
{
	const uint32_t k = f >> 6;
	return k == 0 ? v[0] : k == 1 ? v[1] : k == 2 ? v[2] : v[3];
}

// cnt[f * n_tiles + t] = records of file f in tile t (every entry written: the table needs no zeroing)
__global__ void __launch_bounds__(64) split_count_kernel(const OvlRec *__restrict__ recs, uint64_t n, const uint32_t *__restrict__ file_of,
                                                          uint32_t n_ids, uint32_t n_files, uint64_t n_tiles, uint32_t *__restrict__ cnt,
                                                          uint32_t *__restrict__ bad_cnt)
{
	const uint64_t t = blockIdx.x;
	if (t >= n_tiles) return;
	const int lane = threadIdx.x;
	uint32_t mine[kSplitSlots] = {0, 0, 0, 0}, n_bad = 0;
	for (uint32_t it = 0; it < kSplitIters; ++it) {
		const uint64_t i = t * kSplitTile + it * 64 + (uint32_t)lane;
		bool bad;
		const uint32_t f = split_file(recs, i, n, file_of, n_ids, n_files, &bad);
		const bool ok = i < n && !bad;
		n_bad += (uint32_t)__popcll(__ballot(bad));
		unsigned long long live = __ballot(ok);
		while (live) {
			const uint32_t fc = __shfl(f, __ffsll((long long)live) - 1, 64);
			const unsigned long long m = __ballot(ok && f == fc);
			if (lane == (int)(fc & 63)) {
#pragma unroll
				for (uint32_t k = 0; k < kSplitSlots; ++k) if (k == fc >> 6) mine[k] += (uint32_t)__popcll(m);
			}
			live &= ~m;
		}
	}
#pragma unroll
	for (uint32_t k = 0; k < kSplitSlots; ++k) {
		const uint32_t f = k * 64 + (uint32_t)lane;
		if (f < n_files) cnt[(uint64_t)f * n_tiles + t] = mine[k];
	}
	if (lane == 0 && n_bad) atomicAdd(bad_cnt, n_bad);
}

// cuts[f] = the first output row of file f (first = the exclusive scan of cnt, n_files * n_tiles + 1 entries), cuts[n_files] = all rows
__global__ void split_cuts_kernel(const uint64_t *__restrict__ first, uint64_t n_tiles, uint32_t n_files, uint64_t *__restrict__ cuts)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f <= n_files) cuts[f] = first[(uint64_t)f * n_tiles];
}

// the records to their rows; run only when the count pass found no refused record, so the rows are exactly [0, n)
__global__ void __launch_bounds__(64) split_scatter_kernel(const OvlRec *__restrict__ recs, uint64_t n, const uint32_t *__restrict__ file_of,
                                                            uint32_t n_ids, uint32_t n_files, uint64_t n_tiles, const uint64_t *__restrict__ first,
                                                            OvlRec *__restrict__ out)
{
	const uint64_t t = blockIdx.x;
	if (t >= n_tiles) return;
	const int lane = threadIdx.x;
	unsigned long long run[kSplitSlots];   // next row of the files this lane owns
#pragma unroll
	for (uint32_t k = 0; k < kSplitSlots; ++k) {
		const uint32_t f = k * 64 + (uint32_t)lane;
		run[k] = f < n_files ? first[(uint64_t)f * n_tiles + t] : 0ull;
	}
	for (uint32_t it = 0; it < kSplitIters; ++it) {
		const uint64_t i = t * kSplitTile + it * 64 + (uint32_t)lane;
		bool bad;
		const uint32_t f = split_file(recs, i, n, file_of, n_ids, n_files, &bad);
		const bool ok = i < n && !bad;
		uint4 a = make_uint4(0, 0, 0, 0), b = a;
		if (ok) {
			const uint4 *src = reinterpret_cast<const uint4*>(recs + i);
			a = src[0], b = src[1];
		}
		unsigned long long live = __ballot(ok);
		while (live) {
			const uint32_t fc = __shfl(f, __ffsll((long long)live) - 1, 64);
			const unsigned long long m = __ballot(ok && f == fc);
			const unsigned long long base = __shfl(split_slot(run, fc), (int)(fc & 63), 64);
			if (ok && f == fc) {
				const unsigned long long row = base + (unsigned long long)__popcll(m & ((1ull << lane) - 1));
				if (row < n) {   // (always, when the count pass refused nothing)
					uint4 *dst = reinterpret_cast<uint4*>(out + row);
					dst[0] = a, dst[1] = b;
				}
			}
			if (lane == (int)(fc & 63)) {
#pragma unroll
				for (uint32_t k = 0; k < kSplitSlots; ++k) if (k == fc >> 6) run[k] += (unsigned long long)__popcll(m);
			}
			live &= ~m;
		}
	}
}

// file_of[i] = the file record i of the sort's input belongs to: the last f with fstart[f] <= i (fstart has n_files + 1 entries)
__global__ void file_fill_kernel(const uint64_t *__restrict__ fstart, uint32_t n_files, uint64_t n, uint32_t *__restrict__ file_of)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) file_of[i] = file_of_record(fstart, n_files, i);
}

uint32_t split_tile_records() { return kSplitTile; }
uint32_t split_max_files() { return kSplitMaxFiles; }
void launch_split_count(const OvlRec *recs, uint64_t n, const uint32_t *file_of, uint32_t n_ids, uint32_t n_files, uint64_t n_tiles, uint32_t *cnt,
                        uint32_t *bad_cnt, hipStream_t s)
{
	if (n_tiles) ND_LAUNCH(split_count_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, recs, n, file_of, n_ids, n_files, n_tiles, cnt, bad_cnt);
}
void launch_split_cuts(const uint64_t *first, uint64_t n_tiles, uint32_t n_files, uint64_t *cuts, hipStream_t s)
{
	ND_LAUNCH(split_cuts_kernel, GRID1(n_files + 1), 0, s, first, n_tiles, n_files, cuts);
}
void launch_split_scatter(const OvlRec *recs, uint64_t n, const uint32_t *file_of, uint32_t n_ids, uint32_t n_files, uint64_t n_tiles,
                          const uint64_t *first, OvlRec *out, hipStream_t s)
{
	if (n_tiles) ND_LAUNCH(split_scatter_kernel, dim3((unsigned)n_tiles), dim3(64), 0, s, recs, n, file_of, n_ids, n_files, n_tiles, first, out);
}
void launch_file_fill(const uint64_t *fstart, uint32_t n_files, uint64_t n, uint32_t *file_of, hipStream_t s)
{
	if (n) ND_LAUNCH(file_fill_kernel, GRID1(n), 0, s, fstart, n_files, n, file_of);
}

// ------------------------------------------------------------------------------------------------
// K23: the step-2 writer -- filter_ovl (lib/ovl.c:449-563) and encode_ovl_i (lib/ovl.c:205-253) over the records of one call,
// without the record-by-record pass (host side: ndovl::s2_group / s2_solve in ovlsort_engine.hip, the state in ovl_step2.cpp).
//
// A read is alive before record i while it has looked contained fewer than two times; alive[r] = the number of leading records before
// which read r is alive (0: dead when the call starts, kS2Never: never dies).  With qc(i) / tc(i) = "record i covers its query / target
// end to end within maxhan2", read r is bumped as the query of i when qc(i), and as the target of i when tc(i) and not (qc(i) and the
// query is alive before i); r dies at its (2 - con0)-th bump.  Only the last condition couples reads, and only at records where qc and
// tc both hold: the alive[] of all reads are recomputed from the previous estimate until none changes (s2_events_kernel, one launch a
// round).  Everything else follows from alive[] alone: the verdicts, and per read the end counts, the dovetail maxima, the longest
// internal overlap and the union of the covered intervals.
//
// Every record contributes two entries, 2 * i (its query) and 2 * i + 1 (its target); a stable sort by read name groups them, in
// record order inside a read (a "segment").  The kernels over segments give one wavefront to a segment, 64 entries a step.
constexpr uint32_t kS2Never = 0xffffffffu;
constexpr uint32_t kS2Alive = 1, kS2Lo = 2, kS2Hi = 4, kS2Feed = 8, kS2End3 = 16, kS2Internal = 32;   // bits of an entry's einfo
#define GRIDW(n) dim3((unsigned)(((uint64_t)(n) + 3) / 4)), dim3(256)   // one wavefront per item

// rinfo[i] = qc | tc << 1; flagw[0] |= 1: a span under 21 bases (the stored interval (s + 10, e - 10) would be empty or inverted),
// |= 2: an identity beyond the 15-bit fields -- the call is then the host loop's
__global__ void s2_classify_kernel(const OvlRec10 *__restrict__ recs, uint32_t n, uint32_t h2, uint32_t *__restrict__ ekey,
                                   uint32_t *__restrict__ eval, uint32_t *__restrict__ rinfo, uint32_t *__restrict__ flagw)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const OvlRec10 r = recs[i];
	const uint32_t qc = r.qs <= h2 && r.qe + h2 >= r.qlen, tc = r.ts <= h2 && r.te + h2 >= r.tlen;
	rinfo[i] = qc | tc << 1;
	ekey[2 * i] = r.qname, ekey[2 * i + 1] = r.tname;
	eval[2 * i] = 2 * i, eval[2 * i + 1] = 2 * i + 1;
	uint32_t bad = 0;
	if ((uint64_t)r.qs + 21 > r.qe || (uint64_t)r.ts + 21 > r.te) bad |= 1;
	if (r.identity > 0x7fffu) bad |= 2;
	if (bad) atomicOr(flagw, bad);
}

// head[j] = entry j of the sorted order starts a segment (m entries; head[m] = 0 closes the scan)
__global__ void s2_head_kernel(const uint32_t *__restrict__ skey, uint64_t m, uint32_t *__restrict__ head)
{
	const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j > m) return;
	head[j] = j < m && (j == 0 || skey[j] != skey[j - 1]);
}

// rank = the exclusive scan of head (m + 1 entries): the segments' first entries, names and first records; segof[entry] = its segment
__global__ void s2_segment_kernel(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sval, const uint32_t *__restrict__ head,
                                  const uint64_t *__restrict__ rank, uint64_t m, uint32_t *__restrict__ seg_start, uint32_t *__restrict__ seg_name,
                                  uint32_t *__restrict__ seg_first, uint32_t *__restrict__ segof)
{
	const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j > m) return;
	if (j == m) { seg_start[rank[m]] = (uint32_t)m; return; }
	const uint32_t h = head[j], s = (uint32_t)rank[j] + h - 1;
	segof[sval[j]] = s;
	if (h) seg_start[s] = (uint32_t)j, seg_name[s] = skey[j], seg_first[s] = sval[j];
}

__global__ void s2_init_kernel(const uint32_t *__restrict__ con0, uint32_t d, uint32_t *__restrict__ alive)
{
	const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
	if (s < d) alive[s] = con0[s] >= 2 ? 0u : kS2Never;
}

// One round: alive_new[s] and con[s] (the count after the call, 2 at most) of every segment from alive_old.  The entries of a segment
// are in record order, so the k-th bump is the k-th set bit of the ballots; the wavefront stops there.
__global__ void __launch_bounds__(256) s2_events_kernel(const uint32_t *__restrict__ seg_start, uint32_t d, const uint32_t *__restrict__ sval,
                                                         const uint32_t *__restrict__ rinfo, const uint32_t *__restrict__ segof,
                                                         const uint32_t *__restrict__ con0, const uint32_t *__restrict__ alive_old,
                                                         uint32_t *__restrict__ alive_new, uint32_t *__restrict__ con, uint32_t *__restrict__ changed)
{
	const int lane = threadIdx.x & 63;
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s >= d) return;
	const uint32_t c0 = con0[s];
	uint32_t a = kS2Never, c = c0 < 2 ? c0 : 2;
	if (c0 >= 2) a = 0;
	else {
		const uint64_t j0 = seg_start[s], j1 = seg_start[s + 1];
		uint32_t need = 2 - c0;
		for (uint64_t base = j0; base < j1; base += 64) {
			const uint64_t j = base + lane;
			bool ev = false;
			uint32_t i = 0;
			if (j < j1) {
				const uint32_t e = sval[j];
				i = e >> 1;
				const uint32_t info = rinfo[i];
				if (e & 1) {
					ev = (info & 2) != 0;
					if (ev && (info & 1)) ev = !(i < alive_old[segof[e - 1]]);   // the query took the bump
				} else ev = (info & 1) != 0;
			}
			unsigned long long m = __ballot(ev);
			const uint32_t cnt = (uint32_t)__popcll(m);
			if (cnt >= need) {
				if (need == 2) m &= m - 1;
				a = __shfl(i, __ffsll((long long)m) - 1, 64) + 1;   // alive before that record too, not after it
				c = 2;
				break;
			}
			need -= cnt, c += cnt;
		}
	}
	if (lane == 0) {
		alive_new[s] = a, con[s] = c;
		if (a != alive_old[s]) *changed = 1;
	}
}

// the verdict of record i (the rules of filter_ovl behind the two bumps) and what its two entries feed into their reads
__global__ void s2_verdict_kernel(const OvlRec10 *__restrict__ recs, uint32_t n, uint32_t h1, uint32_t h2, const uint32_t *__restrict__ rinfo,
                                  const uint32_t *__restrict__ segof, const uint32_t *__restrict__ alive, uint32_t *__restrict__ einfo,
                                  uint32_t *__restrict__ keptw, uint8_t *__restrict__ kept)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n) return;
	if (i == n) { keptw[n] = 0; return; }
	const OvlRec10 o = recs[i];
	const uint32_t info = rinfo[i];
	const bool aq = i < alive[segof[2 * i]], at = i < alive[segof[2 * i + 1]];
	const uint32_t q_lo = o.qs, q_hi = o.qlen - o.qe, t_lo = o.ts, t_hi = o.tlen - o.te;
	uint32_t eq = 0, et = 0, v = 0;
	if (aq) eq = kS2Alive | (q_lo <= h2 ? kS2Lo : 0) | (q_hi <= h2 ? kS2Hi : 0);
	if (at) et = kS2Alive | (t_lo <= h2 ? kS2Lo : 0) | (t_hi <= h2 ? kS2Hi : 0);
	if (aq && (info & 1)) v = 0;
	else if (at && (info & 2)) v = 0;
	else if (!aq || !at) v = 0;
	else {
		int q_end = -1, t_end = -1;
		uint32_t gq = 0, gt = 0;
		if (o.rev) {
			if (q_lo <= h1 && t_lo <= h1) q_end = 0, t_end = 0, gq = q_lo, gt = t_lo;
			else if (q_hi <= h1 && t_hi <= h1) q_end = 1, t_end = 1, gq = q_hi, gt = t_hi;
		} else {
			if (q_hi <= h1 && t_lo <= h1) q_end = 1, t_end = 0, gq = q_hi, gt = t_lo;
			else if (q_lo <= h1 && t_hi <= h1) q_end = 0, t_end = 1, gq = q_lo, gt = t_hi;
		}
		if (q_end >= 0) {
			if (gq <= h2 && gt <= h2) eq |= kS2Feed | (q_end ? kS2End3 : 0), et |= kS2Feed | (t_end ? kS2End3 : 0);
			v = 1;
		} else if (o.qs <= h1 && o.qe + h1 >= o.qlen) v = 1;
		else if (o.ts <= h1 && o.te + h1 >= o.tlen) v = 1;
		else eq |= kS2Internal, et |= kS2Internal;
	}
	einfo[2 * i] = eq, einfo[2 * i + 1] = et;
	keptw[i] = v, kept[i] = (uint8_t)v;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) { for (int k = 32; k; k >>= 1) v += __shfl_xor(v, k, 64); return v; }
__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) { for (int k = 32; k; k >>= 1) { const uint32_t o = __shfl_xor(v, k, 64); v = o > v ? o : v; } return v; }
__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
	for (int k = 32; k; k >>= 1) { const unsigned long long o = __shfl_xor(v, k, 64); v = o > v ? o : v; }
	return v;
}

// per read: the counts, the four maxima, the first longest internal overlap and how many intervals it covers while alive (none for a
// read that ends the call dead: it prints nothing but its name)
__global__ void __launch_bounds__(256) s2_reduce_kernel(const uint32_t *__restrict__ seg_start, uint32_t d, const uint32_t *__restrict__ sval,
                                                         const uint32_t *__restrict__ einfo, const OvlRec10 *__restrict__ recs,
                                                         const uint32_t *__restrict__ con, S2ReadOut *__restrict__ out, uint32_t *__restrict__ n_alive)
{
	const int lane = threadIdx.x & 63;
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s > d) return;
	if (s == d) { if (lane == 0) n_alive[d] = 0; return; }
	const uint64_t j0 = seg_start[s], j1 = seg_start[s + 1];
	uint32_t lc = 0, rc = 0, lim = 0, rim = 0, llm = 0, rlm = 0, na = 0;
	unsigned long long best = 0;   // length << 32 | ~entry position: the greatest length, the earliest record among equals
	for (uint64_t j = j0 + lane; j < j1; j += 64) {
		const uint32_t e = sval[j], f = einfo[e];
		if (!(f & kS2Alive)) continue;
		const uint32_t *w = reinterpret_cast<const uint32_t*>(recs + (e >> 1));
		na++, lc += (f & kS2Lo) != 0, rc += (f & kS2Hi) != 0;
		if (f & kS2Feed) {
			const uint32_t qspan = w[3] - w[2], tspan = w[7] - w[6], span = qspan > tspan ? qspan : tspan, ide = w[9];
			if (f & kS2End3) rlm = span > rlm ? span : rlm, rim = ide > rim ? ide : rim;
			else llm = span > llm ? span : llm, lim = ide > lim ? ide : lim;
		}
		if (f & kS2Internal) {
			const uint32_t len = (e & 1) ? w[7] - w[6] : w[3] - w[2];
			const unsigned long long key = (unsigned long long)len << 32 | (uint32_t)~(uint32_t)j;
			if (len && key > best) best = key;
		}
	}
	lc = wave_sum_u32(lc), rc = wave_sum_u32(rc), na = wave_sum_u32(na);
	lim = wave_max_u32(lim), rim = wave_max_u32(rim), llm = wave_max_u32(llm), rlm = wave_max_u32(rlm);
	best = wave_max_u64(best);
	if (lane) return;
	S2ReadOut r = {lc, rc, lim, rim, llm, rlm, 0, 0, na};
	if (best) {
		const uint32_t e = sval[(uint32_t)~(uint32_t)best];
		const uint32_t *w = reinterpret_cast<const uint32_t*>(recs + (e >> 1));
		r.long_s = (e & 1) ? w[6] : w[2], r.long_e = (e & 1) ? w[7] : w[3];
	}
	if (con[s] >= 2) r.n_alive = 0;
	out[s] = r;
	n_alive[s] = r.n_alive;
}

// sort key of entry position j's interval: segment << 32 | start + 10, value: end - 10; all ones for an entry that covers nothing
__global__ void s2_span_keys_kernel(const uint32_t *__restrict__ sval, uint64_t m, const uint32_t *__restrict__ segof,
                                    const uint32_t *__restrict__ einfo, const uint32_t *__restrict__ con, const OvlRec10 *__restrict__ recs,
                                    uint64_t *__restrict__ key, uint64_t *__restrict__ val)
{
	const uint64_t j = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (j >= m) return;
	const uint32_t e = sval[j], s = segof[e];
	const uint32_t *w = reinterpret_cast<const uint32_t*>(recs + (e >> 1));
	const uint32_t a = (e & 1) ? w[6] : w[2], b = (e & 1) ? w[7] : w[3];
	const bool live = (einfo[e] & kS2Alive) && con[s] < 2;
	key[j] = live ? (uint64_t)s << 32 | (uint32_t)(a + 10) : ~0ull;
	val[j] = b - 10;
}

// The union of a read's intervals, sorted by start at [off[s], off[s + 1]): a running maximum of the ends; an interval whose start lies
// beyond it opens a new one (one that starts AT it joins, merge_spans of ovl_step2.cpp).  The merged intervals go to merged[off[s] ..),
// their number to n_merged[s].
__global__ void __launch_bounds__(256) s2_union_kernel(const uint64_t *__restrict__ off, uint32_t d, const uint64_t *__restrict__ key,
                                                        const uint64_t *__restrict__ val, uint2 *__restrict__ merged, uint32_t *__restrict__ n_merged)
{
	const int lane = threadIdx.x & 63;
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s > d) return;
	if (s == d) { if (lane == 0) n_merged[d] = 0; return; }
	const uint64_t j0 = off[s], j1 = off[s + 1];
	uint32_t carry = 0, heads = 0;
	for (uint64_t base = j0; base < j1; base += 64) {
		const uint64_t j = base + lane;
		const bool live = j < j1;
		const uint32_t start = live ? (uint32_t)key[j] : 0u, end = live ? (uint32_t)val[j] : 0u;
		uint32_t run = end;   // inclusive running maximum of the ends
		for (int k = 1; k < 64; k <<= 1) {
			const uint32_t o = __shfl_up(run, k, 64);
			if (lane >= k && o > run) run = o;
		}
		uint32_t before = __shfl_up(run, 1, 64);
		if (lane == 0 || carry > before) before = carry;
		if (carry > run) run = carry;
		const bool head = live && (j == j0 || start > before);
		const bool tail = live && (j + 1 == j1 || (uint32_t)key[j + 1] > run);
		const unsigned long long hm = __ballot(head);
		const uint32_t idx = heads + (uint32_t)__popcll(hm & (~0ull >> (63 - lane))) - 1;
		if (head) merged[j0 + idx].x = start;
		if (tail) merged[j0 + idx].y = run;
		heads += (uint32_t)__popcll(hm);
		carry = __shfl(run, 63, 64);
	}
	if (lane == 0) n_merged[s] = heads;
}

__global__ void __launch_bounds__(256) s2_span_gather_kernel(const uint64_t *__restrict__ off, const uint64_t *__restrict__ dense_off, uint32_t d,
                                                              const uint32_t *__restrict__ n_merged, const uint2 *__restrict__ merged,
                                                              uint2 *__restrict__ dense)
{
	const int lane = threadIdx.x & 63;
	const uint32_t s = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (s >= d) return;
	const uint64_t a = off[s], b = dense_off[s];
	for (uint32_t k = lane; k < n_merged[s]; k += 64) dense[b + k] = merged[a + k];
}

// ---- the 10-field encoder over the kept records
__global__ void s2_compact_kernel(const uint32_t *__restrict__ keptw, const uint64_t *__restrict__ rank, uint32_t n, uint32_t *__restrict__ kidx)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n && keptw[i]) kidx[rank[i]] = i;
}

// put_record10 of ovl_step2.cpp for kept record k (record kidx[k]) behind the kept record in front of it (the first: the caller's prev);
// a lane without a record computes on zeros
__device__ __forceinline__ void encode_fields10(const OvlRec10 *__restrict__ recs, const uint32_t *__restrict__ kidx, uint64_t k, bool live,
                                                uint32_t prev_q, uint32_t prev_t, uint32_t f[10])
{
	OvlRec10 o = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
	uint32_t pq = prev_q, pt = prev_t;
	if (live) {
		o = recs[kidx[k]];
		if (k > 0) { const OvlRec10 *p = recs + kidx[k - 1]; pq = p->qname, pt = p->tname; }
	}
	uint32_t flags = o.rev;
	const uint32_t qspan = o.qe - o.qs, tspan = o.te - o.ts;
	if (o.qname >= pq) f[0] = o.qname - pq; else flags |= 2, f[0] = pq - o.qname;
	if (o.tname >= pt) f[4] = o.tname - pt; else flags |= 4, f[4] = pt - o.tname;
	f[7] = o.qname == pq ? 0 : o.qlen;
	f[8] = o.tname == pt ? 0 : o.tlen;
	if (qspan >= tspan) f[6] = qspan - tspan; else flags |= 8, f[6] = tspan - qspan;
	f[1] = flags & 0xff, f[2] = o.qs, f[3] = qspan, f[5] = o.ts, f[9] = o.identity;
}

// len[k] for k <= n: the bytes of kept record k, 0 behind the last (rank[n] = the number of kept records)
__global__ void s2_size10_kernel(const OvlRec10 *__restrict__ recs, const uint32_t *__restrict__ kidx, const uint64_t *__restrict__ rank, uint32_t n,
                                 uint32_t prev_q, uint32_t prev_t, uint32_t *__restrict__ len)
{
	const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
	if (k > n) return;
	const bool live = k < rank[n];
	uint32_t f[10], nb = 0;
	encode_fields10(recs, kidx, k, live, prev_q, prev_t, f);
#pragma unroll
	for (int x = 0; x < 10; ++x) nb += varint_len(f[x]);
	len[k] = live ? nb : 0;   // 10 .. 47: nine values of up to 5 bytes, the flags of up to 2
}

constexpr uint32_t kEnc10StageWords = (64 * 48 + 3 + 3) / 4 + 1;   // 64 records of up to 47 bytes behind up to 3 bytes of alignment

// off = the exclusive scan of len; out is 4-byte aligned (the staging of codec_write_kernel)
__global__ void __launch_bounds__(64) s2_write10_kernel(const OvlRec10 *__restrict__ recs, const uint32_t *__restrict__ kidx, uint64_t nk,
                                                         uint32_t prev_q, uint32_t prev_t, const uint64_t *__restrict__ off, uint8_t *__restrict__ out)
{
	__shared__ uint32_t stage_w[kEnc10StageWords];
	uint8_t *const stage = reinterpret_cast<uint8_t*>(stage_w);
	const int lane = threadIdx.x;
	const uint64_t k0 = (uint64_t)blockIdx.x * 64, k = k0 + lane;
	const uint64_t k1 = k0 + 64 < nk ? k0 + 64 : nk;
	const uint64_t g0 = off[k0], g1 = off[k1];
	const uint32_t head = (uint32_t)(g0 & 3);
	uint32_t f[10];
	encode_fields10(recs, kidx, k, k < nk, prev_q, prev_t, f);
	if (k < nk) {
		uint32_t at = head + (uint32_t)(off[k] - g0);
#pragma unroll
		for (int x = 0; x < 10; ++x) {
			const uint32_t v = f[x];
			for (int g = (int)varint_len(v) - 1; g >= 0; --g) stage[at++] = (uint8_t)((v >> (7 * g) & 127u) | (g ? 128u : 0u));
		}
	}
	__syncthreads();
	const uint32_t end = head + (uint32_t)(g1 - g0);
	const uint32_t w_lo = (head + 3) & ~3u, w_hi = end & ~3u;
	const uint32_t head_end = w_lo < end ? w_lo : end;
	uint8_t *const base = out + (g0 - head);
	if (head + lane < head_end) base[head + lane] = stage[head + lane];
	for (uint32_t x = w_lo + 4 * (uint32_t)lane; x < w_hi; x += 256) *reinterpret_cast<uint32_t*>(base + x) = stage_w[x >> 2];
	const uint32_t tail = w_hi > head_end ? w_hi : head_end;
	if (tail + lane < end) base[tail + lane] = stage[tail + lane];
}

void launch_s2_classify(const OvlRec10 *recs, uint32_t n, uint32_t h2, uint32_t *ekey, uint32_t *eval, uint32_t *rinfo, uint32_t *flagw, hipStream_t s)
{
	if (n) ND_LAUNCH(s2_classify_kernel, GRID1(n), 0, s, recs, n, h2, ekey, eval, rinfo, flagw);
}
void launch_s2_segments(const uint32_t *skey, const uint32_t *sval, uint64_t m, uint32_t *head, uint64_t *rank, bool second, uint32_t *seg_start,
                        uint32_t *seg_name, uint32_t *seg_first, uint32_t *segof, hipStream_t s)
{
	if (!second) ND_LAUNCH(s2_head_kernel, GRID1(m + 1), 0, s, skey, m, head);
	else ND_LAUNCH(s2_segment_kernel, GRID1(m + 1), 0, s, skey, sval, head, rank, m, seg_start, seg_name, seg_first, segof);
}
void launch_s2_init(const uint32_t *con0, uint32_t d, uint32_t *alive, hipStream_t s)
{
	if (d) ND_LAUNCH(s2_init_kernel, GRID1(d), 0, s, con0, d, alive);
}
void launch_s2_events(const uint32_t *seg_start, uint32_t d, const uint32_t *sval, const uint32_t *rinfo, const uint32_t *segof, const uint32_t *con0,
                      const uint32_t *alive_old, uint32_t *alive_new, uint32_t *con, uint32_t *changed, hipStream_t s)
{
	if (d) ND_LAUNCH(s2_events_kernel, GRIDW(d), 0, s, seg_start, d, sval, rinfo, segof, con0, alive_old, alive_new, con, changed);
}
void launch_s2_verdict(const OvlRec10 *recs, uint32_t n, uint32_t h1, uint32_t h2, const uint32_t *rinfo, const uint32_t *segof, const uint32_t *alive,
                       uint32_t *einfo, uint32_t *keptw, uint8_t *kept, hipStream_t s)
{
	ND_LAUNCH(s2_verdict_kernel, GRID1((uint64_t)n + 1), 0, s, recs, n, h1, h2, rinfo, segof, alive, einfo, keptw, kept);
}
void launch_s2_reduce(const uint32_t *seg_start, uint32_t d, const uint32_t *sval, const uint32_t *einfo, const OvlRec10 *recs, const uint32_t *con,
                      S2ReadOut *out, uint32_t *n_alive, hipStream_t s)
{
	ND_LAUNCH(s2_reduce_kernel, GRIDW((uint64_t)d + 1), 0, s, seg_start, d, sval, einfo, recs, con, out, n_alive);
}
void launch_s2_span_keys(const uint32_t *sval, uint64_t m, const uint32_t *segof, const uint32_t *einfo, const uint32_t *con, const OvlRec10 *recs,
                         uint64_t *key, uint64_t *val, hipStream_t s)
{
	if (m) ND_LAUNCH(s2_span_keys_kernel, GRID1(m), 0, s, sval, m, segof, einfo, con, recs, key, val);
}
void launch_s2_union(const uint64_t *off, uint32_t d, const uint64_t *key, const uint64_t *val, uint2 *merged, uint32_t *n_merged, hipStream_t s)
{
	ND_LAUNCH(s2_union_kernel, GRIDW((uint64_t)d + 1), 0, s, off, d, key, val, merged, n_merged);
}
void launch_s2_span_gather(const uint64_t *off, const uint64_t *dense_off, uint32_t d, const uint32_t *n_merged, const uint2 *merged, uint2 *dense,
                           hipStream_t s)
{
	if (d) ND_LAUNCH(s2_span_gather_kernel, GRIDW(d), 0, s, off, dense_off, d, n_merged, merged, dense);
}
void launch_s2_compact(const uint32_t *keptw, const uint64_t *rank, uint32_t n, uint32_t *kidx, hipStream_t s)
{
	if (n) ND_LAUNCH(s2_compact_kernel, GRID1(n), 0, s, keptw, rank, n, kidx);
}
void launch_s2_size10(const OvlRec10 *recs, const uint32_t *kidx, const uint64_t *rank, uint32_t n, uint32_t prev_q, uint32_t prev_t, uint32_t *len,
                      hipStream_t s)
{
	ND_LAUNCH(s2_size10_kernel, GRID1((uint64_t)n + 1), 0, s, recs, kidx, rank, n, prev_q, prev_t, len);
}
void launch_s2_write10(const OvlRec10 *recs, const uint32_t *kidx, uint64_t nk, uint32_t prev_q, uint32_t prev_t, const uint64_t *off, uint8_t *out,
                       hipStream_t s)
{
	if (nk) ND_LAUNCH(s2_write10_kernel, dim3((unsigned)((nk + 63) / 64)), dim3(64), 0, s, recs, kidx, nk, prev_q, prev_t, off, out);
}

} // namespace ndovl
