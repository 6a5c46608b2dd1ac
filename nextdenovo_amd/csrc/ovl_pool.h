// ovl_pool.h -- what every translation unit of the overlap library shares below the engines (top of ovl_engine.hip): the device block
// pool, the reason of the last failure, the check every device operation goes through and the fault-injection hook.
// hipMalloc / hipFree of multi-GB buffers cost milliseconds each (more when the HBM is nearly full), and every index build / map /
// sort call asks for similar sizes again: the pool takes slabs from the driver and carves the requests out of them.
#pragma once

#include <cstddef>
#include <cstdint>

namespace ndovl {
void *pool_alloc(size_t bytes);   // throws std::runtime_error on failure
void pool_free(void *p);
size_t pool_trim();               // idle slabs back to the driver; returns the bytes released
size_t pool_cached_bytes();       // what the pool holds beyond what is in use
void pool_bytes(uint64_t out[3]);             // in use now, cached for reuse, the most that ever were in use at once
void pool_calls(uint64_t out[2], int reset);  // hipMalloc / hipFree calls the pool made, their wall time in ns

// why the last failed entry point failed (ndgpu_ovl_last_error): 1 = out of device memory, 2 = another device error; taking it clears it
int last_error_take();
void note_oom();

// Every device operation of the overlap library reports its failure by throwing: a rocPRIM primitive that returns an error, a
// kernel launch the runtime refuses.  Until round 4 the primitives' return values were dropped -- and a primitive that fails
// also clears the runtime's sticky error, so the stage-end hipGetLastError() saw nothing: on a device short of memory a sort
// or a scan that never ran left its output buffer as it was and the call returned fewer records, silently.
// Out of memory is noted for ndgpu_ovl_last_error() (1), so that the caller can release memory and try again.
void device_check(int hip_error, const char *what);
// Test hook: NDGPU_OVL_FAIL_AT=k makes the k-th checked device operation of the process (block-pool allocation, rocPRIM primitive,
// kernel launch) fail as if the device were out of memory; read at every operation, so a test can move it between calls.
bool fault_injected();
}
