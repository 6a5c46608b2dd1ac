// ovl_host.h -- host-side support of the overlap library's translation units (internal: nothing here is exported): the one
// error check, the one device buffer, the event timer, the rocPRIM scratch block and the small pieces every C entry point repeats.
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>
#include <vector>

#include <hip/hip_runtime.h>

#include "ovl_device.h"
#include "ovl_pool.h"

// (a device filled to the brim makes the runtime's own allocations fail too -- launch arguments, staging: "out of memory" may
// surface at any call; device_check notes it as what it is, so that the caller can release memory and try again)
#define HIP_OK(e) do { hipError_t _e = (e); if (_e != hipSuccess) { fprintf(stderr, "[ndgpu_overlap] HIP error %s at %s:%d\n", hipGetErrorString(_e), __FILE__, __LINE__); ndovl::device_check((int)_e, "hip call"); } } while (0)

namespace ndovl {

// a block of the pool (ovl_pool.h); the copies and fills cover the buffer's first `count` elements
template <class T> struct DevBuf {
	T *p = nullptr;
	size_t n = 0;
	DevBuf() = default;
	explicit DevBuf(size_t count) { alloc(count); }
	DevBuf(const DevBuf&) = delete;
	DevBuf &operator=(const DevBuf&) = delete;
	DevBuf(DevBuf &&o) noexcept : p(o.p), n(o.n) { o.p = nullptr, o.n = 0; }
	DevBuf &operator=(DevBuf &&o) noexcept { if (this != &o) { release(); p = o.p, n = o.n; o.p = nullptr, o.n = 0; } return *this; }
	~DevBuf() { release(); }
	void alloc(size_t count) { release(); n = count; if (count) p = (T*)pool_alloc(count * sizeof(T)); }
	void release() { if (p) pool_free(p); p = nullptr, n = 0; }
	void upload(const T *src, size_t count, hipStream_t s) { if (count) HIP_OK(hipMemcpyAsync(p, src, count * sizeof(T), hipMemcpyHostToDevice, s)); }
	void download(T *dst, size_t count, hipStream_t s, size_t from = 0) const { if (count) HIP_OK(hipMemcpyAsync(dst, p + from, count * sizeof(T), hipMemcpyDeviceToHost, s)); }
	void zero(size_t count, hipStream_t s) { if (count) HIP_OK(hipMemsetAsync(p, 0, count * sizeof(T), s)); }
	void zero(hipStream_t s) { zero(n, s); }
};

struct EvTimer {
	hipEvent_t a, b;
	hipStream_t s;
	EvTimer(hipStream_t st) : s(st) { HIP_OK(hipEventCreate(&a)); HIP_OK(hipEventCreate(&b)); }
	~EvTimer() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); }
	void start() { HIP_OK(hipEventRecord(a, s)); }
	double stop() { HIP_OK(hipEventRecord(b, s)); HIP_OK(hipEventSynchronize(b)); float ms = 0; HIP_OK(hipEventElapsedTime(&ms, a, b)); return ms; }
};

// a stream of one call: waited for, then destroyed.  Declared after the call's buffers, it ends before they go back to the pool --
// whatever still runs on it when the call fails has finished by then (hipStreamDestroy alone does not wait)
struct StreamGuard { hipStream_t s; ~StreamGuard() { (void)hipStreamSynchronize(s); (void)hipStreamDestroy(s); } };

// The temporary block of the rocPRIM primitives (grow-only: a quarter more than was asked for, plus `pad` bytes) and their two-call
// protocol: called without a block a primitive tells the size it needs and touches nothing; the second call does the work and is a
// checked device operation.  run(prim, false): the size query alone (a primitive over nothing is not called to work).
struct Scratch {
	DevBuf<uint8_t> buf;
	size_t pad;
	explicit Scratch(size_t pad_bytes = 0) : pad(pad_bytes) {}
	void *get(size_t bytes) { if (!buf.p || buf.n < bytes) buf.alloc(bytes + bytes / 4 + pad); return buf.p; }
	template <class F> void run(F &&prim, bool work = true)
	{
		size_t bytes = 0;
		prim(nullptr, bytes);
		if (work) prim(get(bytes), bytes);
	}
};

// The device of an entry point that has no index to take it from: NDGPU_DEVICE (0 when unset; modulo the device count with `wrap`),
// made current.  Returns it, or -1 -- said on stderr -- when the count is looked at and there is no device.
inline int select_device(bool wrap, bool check_count = true)
{
	int n_dev = 0;
	if ((wrap || check_count) && (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)) {
		fprintf(stderr, "[ndgpu_overlap] no HIP device: the overlap library has no CPU path\n");
		return -1;
	}
	int dev = 0;
	if (const char *e = getenv("NDGPU_DEVICE")) dev = atoi(e);
	if (wrap) dev %= n_dev;
	HIP_OK(hipSetDevice(dev));
	return dev;
}

// `n` elements as a malloc block the caller owns (ndgpu_ovl_free); one element's room when there is none, never null
template <class Out, class T> Out *malloc_copy(const T *src, size_t n)
{
	static_assert(sizeof(Out) == sizeof(T), "element layout");
	Out *p = (Out*)malloc(sizeof(T) * std::max<size_t>(n, 1));
	if (!p) throw std::runtime_error("malloc");
	if (n) memcpy(p, src, sizeof(T) * n);
	return p;
}
template <class Out, class T> Out *malloc_copy(const std::vector<T> &v) { return malloc_copy<Out>(v.data(), v.size()); }

// K23: one ndgpu_s2_filter_encode_flags call on the device (ovlsort_engine.hip), in the two steps the run's read table
// (ovl_step2.cpp, the one authority) needs: s2_group names the reads the records touch, the caller looks up how often each has
// looked contained so far, s2_solve computes the rest.  Nothing here knows the table.  Both throw on a device error.
struct S2Call {
	// in
	const OvlRec10 *recs = nullptr;
	uint32_t n = 0, h1 = 0, h2 = 0, prev[2] = {0, 0}, max_rounds = 16;
	uint8_t *kept = nullptr;                    // n verdicts (may be null)
	// out of s2_group: per distinct read, by name: its name and first entry (2 * record + side); order = the reads by first entry
	uint32_t decline = 0;                       // bit 0: a span under 21 bases, bit 1: an identity beyond 15 bits -- nothing else is set then
	std::vector<uint32_t> name, first, order;
	// in of s2_solve
	std::vector<uint32_t> con0;                 // contained count of every read when the call starts
	// out of s2_solve
	bool converged = false;                     // false: the rounds ran out, nothing below is set
	uint32_t rounds = 0;
	std::vector<uint32_t> con;                  // contained count after the call
	std::vector<S2ReadOut> out;
	std::vector<uint64_t> span_off;             // reads + 1 offsets into spans
	std::vector<uint2> spans;                   // the merged intervals (s + 10, e - 10) of the reads alive at the end, ascending
	uint8_t *bytes = nullptr;                   // malloc'd (the caller's to free or hand out)
	uint64_t n_bytes = 0, n_kept = 0;
	uint32_t prev_out[2] = {0, 0};
	uint64_t bytes_up = 0, bytes_down = 0, launches = 0;
	double ms = 0;
	void *dev = nullptr;                        // the call's device buffers between the two steps
};
void s2_group(S2Call &c);
void s2_solve(S2Call &c);
void s2_release(S2Call &c);   // the device buffers, and bytes when the caller has not taken them

} // namespace ndovl
