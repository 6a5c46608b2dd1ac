// ovl_recset.h -- the record set (ndgpu_ovl_recset, include/ndgpu_overlap.h) as the library's translation units see it: made by the
// map (ovl_engine.hip), read by the sorts and cut by the split (ovlsort_engine.hip).  Internal: nothing here is exported.
#pragma once

#include <atomic>
#include <memory>

#include "ovl_device.h"
#include "ovl_host.h"

// records [first, first + n) of a block of the pool.  The block is shared by reference count: the sets a split makes are views into
// one block, which goes back to the pool with the last of them.  A set is never written after it was made.
struct ndgpu_ovl_recset {
	std::shared_ptr<ndovl::DevBuf<ndovl::OvlRec>> buf;   // (none when n == 0)
	uint64_t first = 0, n = 0;
	const ndovl::OvlRec *data() const { return n ? buf->p + first : nullptr; }
};

namespace ndovl {

// ndgpu_ovl_recset_stats: counted where it happens, from any thread
struct RecsetCounters {
	std::atomic<uint64_t> split_ns{0}, sets_made{0}, sets_live{0}, bytes_downloaded{0}, bytes_uploaded{0}, bytes_d2d{0}, split_calls{0},
	                      sets_downloaded{0};
};
inline RecsetCounters g_recset;

inline ndgpu_ovl_recset *recset_view(std::shared_ptr<DevBuf<OvlRec>> buf, uint64_t first, uint64_t n)
{
	ndgpu_ovl_recset *s = new ndgpu_ovl_recset();
	if (n) s->buf = std::move(buf), s->first = first, s->n = n;
	++g_recset.sets_made, ++g_recset.sets_live;
	return s;
}
// a set that owns `buf`, whose first n records are the set
inline ndgpu_ovl_recset *recset_own(DevBuf<OvlRec> &&buf, uint64_t n)
{
	return recset_view(n ? std::make_shared<DevBuf<OvlRec>>(std::move(buf)) : nullptr, 0, n);
}

} // namespace ndovl
