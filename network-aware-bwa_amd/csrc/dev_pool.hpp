// dev_pool.hpp -- device memory of the host units: the per-index pool of working buffers, the staged upload, and the handles
// that own a buffer, an event or a stream.
#pragma once
#include <hip/hip_runtime.h>
#include <mutex>
#include <unordered_map>
#include <vector>
#include "nabwa_internal.hpp"

#pragma GCC visibility push(hidden)      /* internal to libnabwa.so: nothing here joins its dynamic symbols */

/* Working buffers come from a per-index pool: a streaming caller makes one batch after the other, of about the same
 * size, and hipMalloc of the search arena (tens of GB) costs 0.5 - 1 s each time -- more than the search itself.
 * A released buffer is kept (up to NABWA_POOL_GB, default 80: a 10 M-read batch holds about 20 GB, kernel D's page pool 32 GB) and handed to the next request it fits within 25 %;
 * everything cached goes back to the driver when an allocation fails and when the index is destroyed. */
struct nabwa_dev_pool {
	std::mutex mu;
	struct Blk { void *p; size_t bytes; };
	std::vector<Blk> idle;                         /* oldest first */
	std::unordered_map<void*, size_t> live;
	size_t idle_bytes = 0, limit = 0;
	/* staged uploads (pageable caller memory -> pinned slots -> HBM), set up by the first large upload */
	enum { UP_THREADS = 4, UP_SLOT = 32 << 20 };
	uint8_t *pin = 0; hipStream_t up_stream[UP_THREADS] = {}; hipEvent_t up_ev[UP_THREADS][2] = {};
};

nabwa_dev_pool *pool_create();                     /* empty, its limit from NABWA_POOL_GB */
void pool_destroy(nabwa_dev_pool *pl);             /* everything cached and the upload slots back to the driver; the device is set */
void pool_flush(nabwa_dev_pool *pl);               /* caller holds the lock */
hipError_t pool_malloc(nabwa_index *ix, void **out, size_t bytes);
hipError_t pool_free(nabwa_index *ix, void *p);

/* hipMemcpy from pageable memory runs at ~15 GB/s here (one staging thread inside the runtime); four host threads
 * copying into their own pinned slots while the previous slot is in flight reach the link rate.  Jobs: {dst, src, bytes}. */
struct UploadJob { void *dst; const void *src; size_t bytes; };
hipError_t staged_upload(nabwa_index *ix, const UploadJob *jobs, int n_jobs);

/* A buffer from the pool of `ix`, returned to it by release() or when the handle goes.
 * THE RULE: no buffer goes back to the pool while work that uses it may still be in flight -- the pool hands it to the next
 * request at once, without asking the driver.  The normal paths synchronise before they release.  A function that enqueues work
 * on a stream and holds such handles declares a StreamDrain AFTER them: an early return then waits for the stream first. */
template <class T> struct PoolBuf {
	T *p = nullptr; nabwa_index *ix = nullptr;
	PoolBuf() = default;
	PoolBuf(PoolBuf &&o) noexcept : p(o.p), ix(o.ix) { o.p = nullptr; }
	PoolBuf &operator=(PoolBuf &&o) noexcept { if (this != &o) { (void)release(); p = o.p; ix = o.ix; o.p = nullptr; } return *this; }
	PoolBuf(const PoolBuf&) = delete;
	PoolBuf &operator=(const PoolBuf&) = delete;
	~PoolBuf() { (void)release(); }
	hipError_t get(nabwa_index *ix_, size_t bytes) { (void)release(); ix = ix_; return pool_malloc(ix, (void**)&p, bytes); }
	hipError_t release() { T *q = p; p = nullptr; return q ? pool_free(ix, (void*)q) : hipSuccess; }
	operator T*() const { return p; }
};
/* waits for `s` when the scope ends, whatever the result; on a stream that is idle already this returns at once */
struct StreamDrain {
	hipStream_t s;
	~StreamDrain() { (void)hipStreamSynchronize(s); }
};

/* plain hipMalloc memory (hipFree waits for the device by itself) */
struct DevBuf {
	void *p = nullptr;
	DevBuf() = default;
	DevBuf(const DevBuf&) = delete;
	DevBuf &operator=(const DevBuf&) = delete;
	~DevBuf() { (void)release(); }
	int get(size_t bytes) { HIP_CHECK(hipMalloc(&p, bytes ? bytes : 1)); return NABWA_OK; }
	hipError_t release() { void *q = p; p = nullptr; return q ? hipFree(q) : hipSuccess; }
	template <class T> T *as() const { return (T*)p; }
};
struct DevEvent {
	hipEvent_t e = nullptr;
	DevEvent() = default;
	DevEvent(const DevEvent&) = delete;
	DevEvent &operator=(const DevEvent&) = delete;
	~DevEvent() { if (e) (void)hipEventDestroy(e); }
	operator hipEvent_t() const { return e; }
};
struct DevStream {
	hipStream_t s = nullptr;
	DevStream() = default;
	DevStream(const DevStream&) = delete;
	DevStream &operator=(const DevStream&) = delete;
	~DevStream() { if (s) (void)hipStreamDestroy(s); }
	operator hipStream_t() const { return s; }
};

#pragma GCC visibility pop
