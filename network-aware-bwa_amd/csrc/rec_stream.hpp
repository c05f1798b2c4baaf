// rec_stream.hpp -- the host side that the record-stream modules share (bam_sort.hip, nabwa_damage.hip, nabwa_markdup.hip, nabwa_bai.hip;
// DESIGN.md 13): a call's input is n_rec finished BAM records as bytes and in_off[n_rec + 1].  Each module checks what the offsets alone
// say, uploads bytes, offsets and a sentinel, runs its kernels over a persistent grid, brings the lowest damaged record down and says on
// the host what is wrong with it.  What differs -- the structs, the option checks, the kernel sequence, the kinds of damage past the two
// that all look for -- stays in the module.
//
//   fail_fmt             a formatted error of up to three numbers
//   rec_check_offsets    what n_rec, in and in_off say before any handle or device is looked at
//   rec_grow, rec_reserve, rec_reserve_tmp    buffers that only grow, by a quarter more than asked
//   RecStream            device, stream, pinned words, events and the persistent grid of a handle
//   rec_upload           event, bytes, offsets, sentinel, event
//   rec_grid             the workgroups of a call
//   rec_fail_block_size, rec_damaged_head     the messages of the two kinds of damage that every module looks for
#pragma once
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <initializer_list>
#include <utility>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "rec_body.hpp"

#pragma GCC visibility push(hidden)      /* internal to libnabwa.so: nothing here joins its dynamic symbols */

static inline int fail_fmt(int code, const char *fmt, long long a, long long b = 0, long long c = 0)
{
	char m[256]; snprintf(m, sizeof m, fmt, a, b, c);
	return nabwa_fail(code, "%s", m);
}

/* What the arguments alone say, in the order every module has said it.  extra_null: what else of the caller's makes "null argument", tested
 * where the null test stands (the sort's output buffer and capacity).  No handle is looked at: the tests pass any address for one. */
static inline int rec_check_offsets(int64_t n_rec, const uint8_t *in, const int64_t *in_off, bool extra_null = false)
{
	if (n_rec < 0 || n_rec > 0x7fffffff) return fail_fmt(NABWA_EINVAL, "n_rec %lld: 0 .. 2147483647 records", (long long)n_rec);
	if (!in_off || extra_null || (n_rec && !in)) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (in_off[0] < 0) return nabwa_fail(NABWA_EINVAL, "the first offset is negative");
	for (int64_t i = 0; i < n_rec; ++i) {
		if (in_off[i + 1] <= in_off[i]) return fail_fmt(NABWA_EINVAL, "the offsets do not increase at record %lld", (long long)i);
		if (in_off[i + 1] - in_off[i] < REC_MIN_REC) return fail_fmt(NABWA_EINVAL, "record %lld has %lld bytes: a BAM record has at least 36", (long long)i, (long long)(in_off[i + 1] - in_off[i]));
	}
	return NABWA_OK;
}

/* b, which holds `keep` bytes worth keeping, becomes a buffer of at least `bytes`; out of device memory is the caller's to act on (a smaller
 * call).  no_fit: the module's text for that, with one %lld for the bytes */
static inline int rec_grow(DevBuf &b, size_t keep, size_t bytes, hipStream_t st, const char *no_fit)
{
	if (!keep) { const hipError_t e = b.release(); if (e != hipSuccess) return nabwa_hip_fail(e, "hipFree", __FILE__, __LINE__); }
	void *p = nullptr;
	const hipError_t m = hipMalloc(&p, bytes ? bytes : 1);
	if (m == hipErrorOutOfMemory) { (void)hipGetLastError(); return fail_fmt(NABWA_ENOMEM, no_fit, (long long)bytes); }
	if (m != hipSuccess) return nabwa_hip_fail(m, "hipMalloc", __FILE__, __LINE__);
	hipError_t e = hipSuccess;
	if (keep && b.p) { e = hipMemcpyAsync(p, b.p, keep, hipMemcpyDeviceToDevice, st); if (e == hipSuccess) e = hipStreamSynchronize(st); }
	if (e == hipSuccess) e = b.release();
	if (e != hipSuccess) { (void)hipFree(p); return nabwa_hip_fail(e, "moving the arena", __FILE__, __LINE__); }
	b.p = p;
	return NABWA_OK;
}
/* `cap` units of `unit` bytes each in every buffer of `bufs` (what they hold of `have` units is kept) become at least `want`, a quarter more,
 * and `extra` units behind them.  The stream is drained first: a buffer that goes may still be in use */
static inline int rec_reserve(int64_t &cap, int64_t want, int64_t have, hipStream_t st, const char *no_fit, std::initializer_list<std::pair<DevBuf*, int>> bufs, int extra = 0)
{
	if (want <= cap) return NABWA_OK;
	HIP_CHECK(hipStreamSynchronize(st));
	const int64_t to = want + want / 4;
	cap = have;                                                /* (a failure half-way: what is kept still fits every buffer) */
	for (const auto &b : bufs) if (int r = rec_grow(*b.first, (size_t)have * (size_t)b.second, (size_t)(to + extra) * (size_t)b.second, st, no_fit)) return r;
	cap = to;
	return NABWA_OK;
}
/* the scratch of a hipcub call: `cap` bytes of b become at least `want`, a quarter more; nothing in it is kept */
static inline int rec_reserve_tmp(size_t &cap, size_t want, DevBuf &b, hipStream_t st, const char *no_fit)
{
	if (want <= cap) return NABWA_OK;
	HIP_CHECK(hipStreamSynchronize(st));
	cap = 0;
	if (int r = rec_grow(b, 0, want + want / 4, st, no_fit)) return r;
	cap = want + want / 4;
	return NABWA_OK;
}

/* What a handle holds beside its buffers.  A handle declares it before its DevBuf members and calls quiesce() in its destructor's body:
 * the body runs before any member goes, so the stream is drained before the first buffer is freed, as every module's destructor did; the
 * stream itself goes with this member, after the buffers.  (quiesce() and not a destructor of RecStream alone: that would run after the
 * buffers declared behind it, and putting it last would destroy the stream first.) */
struct RecStream {
	enum { MAX_EVENTS = 9 };
	int device = -1, n_blocks = 1;                             /* device: -1 until setup() has set it */
	DevStream st;
	unsigned int *h_words = nullptr;                           /* pinned: the sentinel, and what else a module brings down with it */
	hipEvent_t ev[MAX_EVENTS] = {};
	RecStream() = default;
	RecStream(const RecStream&) = delete;
	RecStream &operator=(const RecStream&) = delete;
	/* the device, a persistent grid of per_cu workgroups of REC_BLOCK threads per compute unit (0: the module has no such grid), a
	 * non-blocking stream, n_words pinned words, n_events <= MAX_EVENTS events.  what: "setting up the ...", for the message */
	int setup(int device_, int per_cu, int n_words, int n_events, const char *what)
	{
		if (n_events > MAX_EVENTS) return fail_fmt(NABWA_EINVAL, "%lld events: a RecStream holds 9", n_events);
		const hipError_t e0 = hipSetDevice(device_);
		if (e0 != hipSuccess) { (void)hipGetLastError(); return nabwa_hip_fail(e0, "hipSetDevice(device)", __FILE__, __LINE__); }      /* (the runtime's last error is not left for a later call to find) */
		device = device_;
		hipError_t e = hipSuccess;
		if (per_cu) {
			int n_cu = 0;
			e = hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, device);
			n_blocks = per_cu * (n_cu > 0 ? n_cu : 1);
		}
		if (e == hipSuccess) e = hipStreamCreateWithFlags(&st.s, hipStreamNonBlocking);
		if (e == hipSuccess) e = hipHostMalloc((void**)&h_words, (size_t)n_words * sizeof(unsigned int), hipHostMallocDefault);
		for (int k = 0; k < n_events && e == hipSuccess; ++k) e = hipEventCreate(&ev[k]);
		return e == hipSuccess ? NABWA_OK : nabwa_hip_fail(e, what, __FILE__, __LINE__);
	}
	void quiesce()
	{
		if (device < 0) return;
		(void)hipSetDevice(device);
		if (st.s) (void)hipStreamSynchronize(st.s);
		if (h_words) (void)hipHostFree(h_words);
		h_words = nullptr;
		for (hipEvent_t &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
	}
};

/* ev[0], the records' bytes, their offsets, n_words sentinel words from the pinned h_sentinel to d_sentinel, ev[1] */
static inline int rec_upload(RecStream &rs, DevBuf &d_in, DevBuf &d_off, void *d_sentinel, const unsigned int *h_sentinel, int n_words, int64_t n_rec, const uint8_t *in, const int64_t *in_off)
{
	const int64_t base = in_off[0], total = in_off[n_rec] - base;
	hipStream_t st = rs.st;
	HIP_CHECK(hipEventRecord(rs.ev[0], st));
	HIP_CHECK(hipMemcpyAsync(d_in.p, in + base, (size_t)total, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(d_off.p, in_off, (size_t)(n_rec + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(d_sentinel, h_sentinel, (size_t)n_words * sizeof(unsigned int), hipMemcpyHostToDevice, st));
	HIP_CHECK(hipEventRecord(rs.ev[1], st));
	return NABWA_OK;
}

/* the workgroups of a call of n_rec records, `groups` per workgroup and trip: no more than there are trips */
static inline int rec_grid(int64_t n_rec, int groups, int n_blocks)
{
	const int64_t trips = (n_rec + groups - 1) / groups;
	return (int)(trips < n_blocks ? trips : n_blocks);
}

static inline int rec_fail_block_size(int64_t i, int64_t says, int64_t size)
{
	return fail_fmt(NABWA_EDATA, "record %lld: its block_size says %lld bytes, its offsets %lld", (long long)i, (long long)says, (long long)size);
}
/* Record i, which a kernel found damaged, from its bytes on the host, for the message: non-zero and the error set for the two kinds of
 * damage that every module looks for (REC_HEAD), 0 where it is the module's to say */
static inline int rec_damaged_head(int64_t i, const uint8_t *rec, int64_t size)
{
	if ((int64_t)rec_u32(rec) + 4 != size) return rec_fail_block_size(i, (int64_t)rec_u32(rec) + 4, size);
	REC_FIELDS(rec);
	const uint64_t need = REC_NEED(l_name, n_cig, L);
	if (need > (uint64_t)size) return fail_fmt(NABWA_EDATA, "record %lld: its name, CIGAR, bases and qualities need %lld bytes, it has %lld", (long long)i, (long long)need, (long long)size);
	return 0;
}

#pragma GCC visibility pop
