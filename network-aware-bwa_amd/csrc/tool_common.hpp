// tool_common.hpp -- what the command-line tools (nabwa_aln, nabwa_bam2bam, nabwa_samse / nabwa_sampe, nabwa_worker, nabwa_index) share:
// how a run ends, which GPU(s) it uses, index replicas, final_rename, the version string, and the two ways threads hand work
// to each other (Chan, InOrder).  Host code only.  The including program defines, before including this header,
//   TOOL              its name as its messages carry it, e.g. "nabwa_aln"
//   TOOL_DIE_STATUS   the exit status of die() if it is not 1
//   TOOL_FAIL_THROWS  if fail() is to throw BadInput (a tool whose main thread reports what its helper threads met) and not to exit
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <condition_variable>
#include <deque>
#include <map>
#include <mutex>
#include <string>
#include <thread>
#include <vector>
#include "../../include/nabwa.h"
#include "host_util.hpp"

#ifndef TOOL
#error "define TOOL (the program's name in its messages) before including tool_common.hpp"
#endif
#ifndef TOOL_DIE_STATUS
#define TOOL_DIE_STATUS 1
#endif

/* the VN: of the @PG line the tools write */
static const char *const VERSION = "0.5.10-evan.6.3+nabwa";

/* any thread may end the run: no exit handlers (they would tear the GPU runtime down under the other threads) */
[[noreturn]] static inline void die(const char *what, const char *why) { fprintf(stderr, "[" TOOL "] %s: %s\n", what, why); fflush(stderr); _exit(TOOL_DIE_STATUS); }

/* input the tool cannot take: exit status 1 */
struct BadInput { std::string msg; };
#ifdef TOOL_FAIL_THROWS
[[noreturn]] static inline void fail(const std::string &msg) { throw BadInput{ msg }; }
#else
[[noreturn]] static inline void fail(const std::string &msg) { fprintf(stderr, "[" TOOL "] %s\n", msg.c_str()); exit(1); }
#endif

/* an integer of the environment, at least lo and at most INT_MAX; unset or empty: dflt */
static inline int env_int(const char *name, int dflt, int lo)
{
	const char *v = getenv(name);
	if (!v || !*v) return dflt;
	const long x = strtol(v, 0, 10);
	return x < lo ? lo : x > 0x7fffffff ? 0x7fffffff : (int)x;
}

/* NABWA_DEDUP / NABWA_DEDUP_HASH_BITS as nabwa_batch_create reads them (include/nabwa.h): a value it would refuse is refused by the tool
 * before the index is loaded.  False after the line that says so; the caller leaves with status 1 */
static inline bool tool_dedup_ok()
{
	const char *e = getenv("NABWA_DEDUP");
	const bool on = e && strcmp(e, "0");
	if (on && strcmp(e, "1")) { fprintf(stderr, "[" TOOL "] NABWA_DEDUP=%s: 0 or 1\n", e); return false; }
	if (const char *k = on ? getenv("NABWA_DEDUP_HASH_BITS") : 0) {
		char *end = 0;
		const long v = strtol(k, &end, 10);
		if (end == k || *end || v < 0 || v > 64) { fprintf(stderr, "[" TOOL "] NABWA_DEDUP_HASH_BITS=%s: 0..64\n", k); return false; }
	}
	/* NABWA_DEDUP_CACHE: a number of MiB, and a positive one only behind NABWA_DEDUP=1 (whether the device has that much free is the library's to say) */
	if (const char *k = getenv("NABWA_DEDUP_CACHE")) {
		char *end = 0;
		const long v = strtol(k, &end, 10);
		if (end == k || *end || v < 0) { fprintf(stderr, "[" TOOL "] NABWA_DEDUP_CACHE=%s: a number of MiB, 0 for off\n", k); return false; }
		if (v > 0 && !on) { fprintf(stderr, "[" TOOL "] NABWA_DEDUP_CACHE=%s needs NABWA_DEDUP=1\n", k); return false; }
	}
	return true;
}

/* the one line a tool ends with when NABWA_DEDUP_CACHE was on: the read caches of its index replicas, summed */
static inline void tool_dedup_cache_summary(const std::vector<nabwa_index_t*> &ixs)
{
	uint64_t sum[8] = { 0 };
	for (nabwa_index_t *ix : ixs) {
		uint64_t v[8];
		if (ix && nabwa_index_dedup_cache_stats(ix, v) == NABWA_OK) for (int q = 0; q < 8; ++q) sum[q] += v[q];
	}
	if (sum[0]) fprintf(stderr, "[" TOOL "] dedup cache: %llu reads given, %llu searched, %llu served, %llu entries, %llu of %llu bytes\n", (unsigned long long)sum[4],
						(unsigned long long)(sum[4] - sum[5]), (unsigned long long)sum[5], (unsigned long long)sum[2], (unsigned long long)sum[1], (unsigned long long)sum[0]);
}

/* threads of the BGZF block work, in and out: the cores, at most 16 (host_threads() without NABWA_HOST_THREADS, which these never read) */
static inline int io_threads() { int nt = (int)std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16; return nt; }

/* NABWA_DEVICE or 0 into *device.  False when that is none of the visible GPUs, after the line that says so; the caller leaves with
 * status 2.  tail: what the tool adds to the line; null: say nothing (nabwa_index looks at its input first) */
static inline bool tool_device(int *device, const char *tail)
{
	*device = env_int("NABWA_DEVICE", 0);
	const int ndev = nabwa_device_count();
	if (*device >= 0 && *device < ndev) return true;
	if (tail) fprintf(stderr, "[" TOOL "] no usable GPU (NABWA_DEVICE=%d, %d device(s) visible)%s\n", *device, ndev, tail);
	return false;
}

/* the GPUs of NABWA_DEVICES ("0,1,2,3"; read up to the first thing that is no number, so "1,,2" is 1); none there: NABWA_DEVICE or 0 */
static inline std::vector<int> tool_devices()
{
	std::vector<int> devices;
	if (getenv("NABWA_DEVICES"))
		for (const char *q = getenv("NABWA_DEVICES"); *q; ) { char *e; const long d = strtol(q, &e, 10); if (e == q) break; devices.push_back((int)d); q = *e == ',' ? e + 1 : e; }
	if (devices.empty()) devices.push_back(env_int("NABWA_DEVICE", 0));
	return devices;
}

/* one index replica per device, loaded side by side.  -1: all of ixs are loaded; else the first g whose load failed, err says why, and
 * nothing stays loaded */
static inline int load_replicas(const char *prefix, const std::vector<int> &devices, int with_sa, int with_ref, std::vector<nabwa_index_t*> &ixs, std::string &err)
{
	ixs.assign(devices.size(), nullptr);
	std::vector<std::string> errs(devices.size());
	std::vector<std::thread> th;
	for (size_t g = 0; g < devices.size(); ++g)
		th.emplace_back([&, g]() { if (nabwa_index_load(prefix, devices[g], with_sa, with_ref, &ixs[g]) != NABWA_OK) { errs[g] = nabwa_last_error(); ixs[g] = nullptr; } });
	for (auto &x : th) x.join();
	for (size_t g = 0; g < devices.size(); ++g)
		if (!ixs[g]) {
			err = errs[g];
			for (nabwa_index_t *&p : ixs) if (p) { nabwa_index_destroy(p); p = nullptr; }
			return (int)g;
		}
	return -1;
}

/* final_rename (utils.c:159-173): every trailing '_' of the output's name goes once the file is complete ("out.bam__" becomes
 * "out.bam") -- unless nothing would be left of the name or of its last path component.  check: a rename that fails ends the run */
static inline void final_rename(const char *ofile, bool check)
{
	if (!ofile) return;
	std::string to(ofile);
	size_t e = to.size();
	while (e > 0 && to[e - 1] == '_') --e;
	if (e == 0 || to[e - 1] == '/' || e == to.size()) return;
	to.resize(e);
	fprintf(stderr, "[" TOOL "] finished, renaming %s to %s.\n", ofile, to.c_str());
	if (rename(ofile, to.c_str()) != 0 && check) die(ofile, "cannot rename");
}

/* a bounded queue between two threads */
template <class T> struct Chan {
	std::mutex m; std::condition_variable cv; std::deque<T> q; size_t cap; bool closed;
	explicit Chan(size_t cap_) : cap(cap_), closed(false) {}
	void put(T &&x) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return q.size() < cap; }); q.push_back(std::move(x)); cv.notify_all(); }
	bool get(T &x) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return !q.empty() || closed; }); if (q.empty()) return false; x = std::move(q.front()); q.pop_front(); cv.notify_all(); return true; }
	void close() { std::unique_lock<std::mutex> l(m); closed = true; cv.notify_all(); }
};

/* results of several workers, out in the order of their sequence numbers 0, 1, 2, ...: put(seq, x) from any thread, get(x) on one.  put
 * waits while seq is `ahead` or more past the number get() hands out next, so at most `ahead` results wait here.  close(): no put will
 * follow, get() returns false once everything is out.  fail(): the run is lost; every put and get, waiting or yet to come, returns false */
template <class T> struct InOrder {
	std::mutex m; std::condition_variable cv; std::map<long, T> held; long next, ahead; bool closed, lost;
	explicit InOrder(long ahead_) : next(0), ahead(ahead_), closed(false), lost(false) {}
	bool put(long seq, T &&x) { std::unique_lock<std::mutex> l(m); cv.wait(l, [&] { return lost || seq - next < ahead; }); if (lost) return false; held.emplace(seq, std::move(x)); cv.notify_all(); return true; }
	bool get(T &x)
	{
		std::unique_lock<std::mutex> l(m);
		cv.wait(l, [&] { return lost || closed || held.count(next); });
		if (lost || !held.count(next)) return false;
		x = std::move(held[next]); held.erase(next); ++next;
		cv.notify_all();
		return true;
	}
	void close() { std::unique_lock<std::mutex> l(m); closed = true; cv.notify_all(); }
	void fail() { std::unique_lock<std::mutex> l(m); lost = true; cv.notify_all(); }
	bool failed() { std::unique_lock<std::mutex> l(m); return lost; }
};
