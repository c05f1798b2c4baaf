// host_util.hpp -- the library's host plumbing: the last error, the NABWA_TIMING clock, integer switches of the environment and slices of independent records on host threads.
#pragma once
#include <stdlib.h>
#include <chrono>
#include <thread>
#include <vector>

/* the library's last error (nabwa_api.hip): keeps the message for nabwa_last_error and returns `code`.  Declared here for the units that
 * are host code only; the tools, which share this header, never call it. */
int nabwa_fail(int code, const char *fmt, const char *a = "");

/* wall clock of the NABWA_TIMING lines, in seconds */
static inline double now_s() { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

/* an integer switch of the environment; unset or empty: dflt */
static inline int env_int(const char *name, int dflt)
{
	const char *s = getenv(name);
	return s && *s ? atoi(s) : dflt;
}

/* threads for n independent records: the cores, at most 16, or NABWA_HOST_THREADS (a value below 1 counts as 1); one thread
 * when n < min_n.  min_n is 4096 in the SE / PE finishing chains and refine_batch, 8192 in the BAM front-end, 65536 in
 * nabwa_isize_add_pairs. */
static inline int host_threads(size_t n, size_t min_n)
{
	int nt = (int)std::thread::hardware_concurrency(); if (nt < 1) nt = 1; if (nt > 16) nt = 16;
	if (const char *e = getenv("NABWA_HOST_THREADS")) nt = atoi(e) > 0 ? atoi(e) : 1;
	if (n < min_n) nt = 1;
	return nt;
}

/* f(slice, lo, hi) on nt even slices of [0, count); slice t is [count t / nt, count (t + 1) / nt).  One slice runs on the caller. */
template <class F> static inline void host_parallel(int nt, size_t count, F f)
{
	if (nt <= 1) { f(0, (size_t)0, count); return; }
	std::vector<std::thread> th;
	for (int t = 0; t < nt; ++t) th.emplace_back([=]() { f(t, count * t / nt, count * (t + 1) / nt); });
	for (auto &x : th) x.join();
}
