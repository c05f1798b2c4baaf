// host_pool.cpp -- the idle list of host_pool.hpp.
#include <sys/mman.h>
#include <mutex>
#include <utility>
#include <vector>
#include "host_pool.hpp"

static std::mutex g_res_mu;
/* never destroyed: a batch may be given back while the process winds down, after the statics of this file would be gone, and the idle
 * blocks stay reachable to the end (a leak checker sees them as what they are, memory held on purpose) */
static std::vector<std::pair<void*, size_t>> &g_res_idle = *new std::vector<std::pair<void*, size_t>>();

void *res_take(size_t bytes)
{
	{
		std::lock_guard<std::mutex> lk(g_res_mu);
		for (size_t i = 0; i < g_res_idle.size(); ++i)
			if (g_res_idle[i].second >= bytes && g_res_idle[i].second <= 2 * bytes + (1u << 20)) { void *p = g_res_idle[i].first; g_res_idle.erase(g_res_idle.begin() + i); return p; }
	}
	/* large blocks on 2 MB boundaries with the huge-page advice: the passes touch a line or two of every 3 KB record, and with
	 * 4 KB pages nearly each of those touches was a TLB miss as well */
	if (bytes >= ((size_t)64 << 20)) {
		void *p = 0;
		const size_t al = (size_t)2 << 20, sz = (bytes + al - 1) / al * al;
		if (posix_memalign(&p, al, sz) == 0) { (void)madvise(p, sz, MADV_HUGEPAGE); return p; }
	}
	return malloc(bytes);
}

void res_give(void *p, size_t bytes)
{
	if (!p) return;
	std::lock_guard<std::mutex> lk(g_res_mu);
	size_t tot = bytes;
	for (auto &x : g_res_idle) tot += x.second;
	if (tot > ((size_t)16 << 30) || g_res_idle.size() >= 24) { free(p); return; }      /* (a pipeline holds four batches: two 3 GB record blocks and a dozen smaller ones come and go) */
	g_res_idle.push_back({ p, bytes });
}
