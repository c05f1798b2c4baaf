// host_pool.hpp -- the pool of per-batch host blocks behind the BAM front-end, and the one type that owns a block from it.
// A streaming caller makes one batch after the other, and fresh memory costs a page fault per 3 KB record (0.4 s per million): the
// blocks of a finished batch are kept (up to 16 GB, 24 blocks) and handed to the next one.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>

/* a block of at least `bytes` bytes: an idle one of bytes .. 2 * bytes + 1 MB when there is one, else fresh memory -- from 64 MB up on a
 * 2 MB boundary with MADV_HUGEPAGE.  Null when there is no memory. */
void *res_take(size_t bytes);
/* the block back to the idle list, or to the system when the list is full; `bytes` is what it was taken with */
void res_give(void *p, size_t bytes);

/* A block from the pool as raw memory for T: nothing is constructed or destroyed here, only what its user fills is valid.  take() gives back
 * what was held before; give() may be called any time and the destructor calls it. */
template <class T> struct Pooled {
	T *p; size_t bytes;
	Pooled() : p(0), bytes(0) {}
	~Pooled() { give(); }
	Pooled(const Pooled&) = delete;
	Pooled &operator=(const Pooled&) = delete;
	bool take(size_t b) { give(); p = (T*)res_take(b); bytes = p ? b : 0; return p != 0; }
	void give() { res_give(p, bytes); p = 0; bytes = 0; }
	void swap(Pooled &o) { T *const q = p; p = o.p; o.p = q; const size_t b = bytes; bytes = o.bytes; o.bytes = b; }
	explicit operator bool() const { return p != 0; }
	T *get() const { return p; }
	T &operator[](size_t i) const { return p[i]; }
};

/* bytes without the zero fill of std::vector (100 MB per million reads, written once by many threads); from 1 MB up they are a block of the
 * pool: no page faults, no unmapping from batch to batch */
struct RawBytes {
	Pooled<uint8_t> blk; uint8_t *p; size_t n, cap;
	RawBytes() : p(0), n(0), cap(0) {}
	~RawBytes() { drop(); }
	RawBytes(const RawBytes&) = delete;
	RawBytes &operator=(const RawBytes&) = delete;
	void drop() { if (blk) blk.give(); else free(p); p = 0; n = cap = 0; }
	bool alloc(size_t m)
	{
		drop();
		cap = m ? m : 1;
		if (cap >= ((size_t)1 << 20)) { blk.take(cap); p = blk.get(); } else p = (uint8_t*)malloc(cap);
		n = m;
		if (!p) cap = 0;
		return p != 0;
	}
	uint8_t *data() { return p; }
	const uint8_t *data() const { return p; }
	const uint8_t *begin() const { return p; }
};
