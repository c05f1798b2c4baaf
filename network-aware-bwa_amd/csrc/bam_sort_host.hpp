// bam_sort_host.hpp -- NABWA_SORT=host of `nabwa_bam2bam --sort`: what nabwa_bam_sort_run computes (include/nabwa.h), on host
// threads -- the same keys, a stable sort of (key, index), a gather with memcpy -- so that the tool's two settings give identical bytes and
// the GPU path has something to be measured against.  Host code only; part of the tool, not of the library (the library has no CPU path).
#pragma once
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <thread>
#include <utility>
#include <vector>
#include "../../include/nabwa.h"

/* records in[off[i] .. off[i + 1]), i < n, each of at least 36 bytes -> out, out_off (n + 1), keys_out (n) and perm_out (n, may be null) as
 * nabwa_bam_sort_run_ex gives them, by nt threads.  Returns -1, or the lowest record whose block_size is not what its offsets say (nothing is written to out then) */
static inline int64_t bam_sort_host(int nt, int64_t n, const uint8_t *in, const int64_t *off, uint8_t *out, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out = nullptr)
{
	typedef std::pair<uint64_t, uint32_t> KI;
	if (nt < 1) nt = 1;
	if ((int64_t)nt > n) nt = n > 0 ? (int)n : 1;
	auto each = [&](auto f) { std::vector<std::thread> th; for (int t = 0; t < nt; ++t) th.emplace_back(f, t); for (auto &x : th) x.join(); };
	auto lo_of = [&](int t) { return n * t / nt; };
	std::vector<KI> a((size_t)n), b((size_t)n);
	std::vector<int64_t> bad((size_t)nt, -1);
	each([&](int t) {          /* the keys of a slice, and the slice sorted: indices rise within equal keys */
		for (int64_t i = lo_of(t); i < lo_of(t + 1); ++i) {
			const uint8_t *r = in + off[i];
			uint32_t bs; int32_t tid, pos;
			memcpy(&bs, r, 4); memcpy(&tid, r + 4, 4); memcpy(&pos, r + 8, 4);
			if ((int64_t)bs + 4 != off[i + 1] - off[i] && bad[(size_t)t] < 0) bad[(size_t)t] = i;
			a[(size_t)i] = KI((uint64_t)(uint32_t)tid << 32 | (uint32_t)((uint32_t)pos + 1u), (uint32_t)i);
		}
		std::stable_sort(a.begin() + lo_of(t), a.begin() + lo_of(t + 1), [](const KI &x, const KI &y) { return x.first < y.first; });
	});
	for (int64_t x : bad) if (x >= 0) return x;
	/* merge neighbouring slices, rounds of twice the width; std::merge takes the left slice's element on a tie: the lower index */
	for (int w = 1; w < nt; w *= 2) {
		each([&](int t) {
			if (t % (2 * w)) return;
			const int64_t lo = lo_of(t), mid = lo_of(t + w < nt ? t + w : nt), hi = lo_of(t + 2 * w < nt ? t + 2 * w : nt);
			std::merge(a.begin() + lo, a.begin() + mid, a.begin() + mid, a.begin() + hi, b.begin() + lo, [](const KI &x, const KI &y) { return x.first < y.first; });
		});
		a.swap(b);
	}
	std::vector<int64_t> oo((size_t)n + 1);
	oo[0] = 0;
	for (int64_t j = 0; j < n; ++j) { const uint32_t i = a[(size_t)j].second; oo[(size_t)j + 1] = oo[(size_t)j] + (off[i + 1] - off[i]); }
	each([&](int t) {
		for (int64_t j = lo_of(t); j < lo_of(t + 1); ++j) {
			const uint32_t i = a[(size_t)j].second;
			memcpy(out + oo[(size_t)j], in + off[i], (size_t)(off[i + 1] - off[i]));
			if (keys_out) keys_out[j] = a[(size_t)j].first;
			if (perm_out) perm_out[j] = i;
		}
	});
	if (out_off) memcpy(out_off, oo.data(), sizeof(int64_t) * ((size_t)n + 1));
	return -1;
}

/* the k-way merge of sorted runs by their key arrays alone: calls take(run, record) for every record of every run in non-decreasing key
 * order, a tie going to the earlier run (and, within a run, to the earlier record) -- the stable sort of the runs laid end to end */
template <class F> static inline void bam_sort_merge(const std::vector<const std::vector<uint64_t>*> &keys, F take)
{
	const size_t k = keys.size();
	std::vector<size_t> at(k, 0);
	typedef std::pair<uint64_t, size_t> KR;                    /* (key, run): the pair's own order is the tie rule */
	std::vector<KR> heap;
	auto after = [](const KR &x, const KR &y) { return x > y; };
	for (size_t r = 0; r < k; ++r) if (!keys[r]->empty()) heap.push_back(KR((*keys[r])[0], r));
	std::make_heap(heap.begin(), heap.end(), after);
	while (!heap.empty()) {
		std::pop_heap(heap.begin(), heap.end(), after);
		const size_t r = heap.back().second;
		heap.pop_back();
		/* this run goes on while its next key is not beyond the best of the others */
		const std::vector<uint64_t> &kr = *keys[r];
		for (;;) {
			take(r, at[r]);
			if (++at[r] == kr.size()) break;
			const KR next(kr[at[r]], r);
			if (!heap.empty() && after(next, heap.front())) { heap.push_back(next); std::push_heap(heap.begin(), heap.end(), after); break; }
		}
	}
}
