// nabwa_batch.hip -- one batch of reads through the search: upload and re-layout, kernels W and S, the hand-over of the searches
// kernel S flags to kernel D (nabwa_batch_deep.hip), and the read-back of the hits.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <mutex>
#include <vector>
#include "../../include/nabwa.h"
#include "nabwa_batch.hpp"
#include "dedup_cache_body.hpp"
#include "host_util.hpp"

static void layout(SearchParams &P, uint32_t cap, int max_len, int seed_len, uint32_t NS)
{
	// per-read width record
	P.WL = align_up((uint32_t)max_len + 1, 16);
	P.WLB = P.WL + 16;
	P.SLB = align_up((uint32_t)(max_len > seed_len ? seed_len : 0) + 1, 16) + 16;      /* seed bounds exist only for reads longer than the seed (bwtaln.c:126-130) */
	P.woff_bid = 2 * P.WL * 4;
	P.woff_sbid = P.woff_bid + 2 * P.WLB;
	P.wstride = align_up(P.woff_sbid + 2 * P.SLB, 64);
	// per-lane search scratch
	P.cap = cap; P.NS = NS;
	P.lane_stride = align_up((size_t)cap * 16, 64);
}

extern "C" void nabwa_batch_destroy(nabwa_batch_t *b)
{
	if (!b) return;
	(void)hipSetDevice(b->ix->device);
	if (b->stream) (void)hipStreamSynchronize(b->stream);      /* the buffers go back to the pool, not to the driver: nothing may still use them */
	if (b->cache_pinned) { std::lock_guard<std::mutex> lk(b->cache->mu); --b->cache->pins; }      /* its references into the read cache go with it */
	delete b;
}

namespace {
/* what nabwa_batch_create derives on the host from the option block and the read lengths */
struct BatchShape {
	int max_len = 0, min_len = 65535; int64_t padded_total = 0;
	std::vector<uint8_t> md_tab, mg_tab;     /* by read length: what the search of such a read runs with */
	uint32_t NS = 1, NS1 = 1;                /* score levels: the reference's formula; those the first pass can address */
	bool deep_only = false;
};
}

// ---- step 1 of nabwa_batch_create: per-read option derivation, on the host in double (bwtaln.c:102-106,125), and its refusals
static int derive_options(const nabwa_gap_opt_t *opt, int n, const int64_t *off, int per_read, BatchShape &s)
{
	// One threaded pass over the read boundaries: validity, the lengths that occur, the padded size.  Everything per read
	// that follows from its length alone (max_diff, max_gapo) is a table over lengths, applied on the device.
	bool bad_len = false;
	std::vector<uint8_t> seen(65536, 0);
	{
		const int NT = n >= (1 << 20) ? 4 : 1;
		struct Part { int mx = 0, mn = 65535; int64_t padded = 0; bool bad = false; std::vector<uint8_t> seen; };
		std::vector<Part> part(NT);
		for (Part &q : part) q.seen.assign(65536, 0);
		host_parallel(NT, (size_t)n, [&](int t, size_t i0, size_t i1) {
			Part &q = part[t];
			for (size_t i = i0; i < i1; ++i) {
				const int64_t L = off[i + 1] - off[i];
				if (L < 0 || L > 65535) { q.bad = true; continue; }
				q.seen[L] = 1; q.padded += (L + 15) / 16 * 16;
				if (L > q.mx) q.mx = (int)L;
				if (L < q.mn) q.mn = (int)L;
			}
		});
		for (auto &q : part) {
			bad_len |= q.bad; s.padded_total += q.padded;
			if (q.mx > s.max_len) s.max_len = q.mx;
			if (q.mn < s.min_len) s.min_len = q.mn;
			for (int L = 0; L < 65536; ++L) seen[L] |= q.seen[L];
		}
	}
	if (bad_len) return nabwa_fail(NABWA_EINVAL, "read length outside 0..65535");
	std::vector<int> md_of(s.max_len + 1, opt->max_diff);
	if (opt->fnr > 0.0f) for (int L = 0; L <= s.max_len; ++L) md_of[L] = nabwa_cal_maxdiff(L, 0.02, opt->fnr);
	s.md_tab.assign(s.max_len + 1, 0); s.mg_tab.assign(s.max_len + 1, 0);
	int mdx = 0, mgx = 0;
	for (int L = 0; L <= s.max_len; ++L) {
		if (!seen[L]) continue;
		const int md_sizing = md_of[per_read ? L : s.max_len];
		int g = opt->max_gapo; if (md_sizing < g) g = md_sizing;
		const int d = md_of[L];
		/* kernel D's entries keep n_mm / n_gapo / n_gape in 8 bits each, the bound bytes of kernel W hold min(bid, 127) */
		if (d < 0 || d > 126 || g < 0 || g > 255) return nabwa_fail(NABWA_EINVAL, "max_diff > 126 or max_gapo > 255 (unsupported)");
		s.md_tab[L] = (uint8_t)d; s.mg_tab[L] = (uint8_t)g;
		if (d > mdx) mdx = d;
		if (g > mgx) mgx = g;
		const long ns = (long)(md_sizing + 1) * opt->s_mm + (long)(g + 1) * opt->s_gapo + (long)(opt->max_gape + 1) * opt->s_gape;
		if (ns > (long)s.NS) s.NS = (uint32_t)ns;
	}
	/* First pass: score levels that can actually hold an entry.  A child is only made of a parent that passed the
	 * m >= 0 test (bwtgap.c:152-154), so it has at most max_diff + 1 counted differences, at most max_gapo opens and
	 * max_gape extensions; its score is the largest index the per-score lists are addressed with.  (The formula above
	 * is the reference's initial best_score, a value that is compared, never an index; the second pass still sizes by it.) */
	{
		const bool gape_counts = opt->mode & NABWA_MODE_GAPE;
		for (int a = 0; a <= mdx + 1; ++a)
			for (int g = 0; g <= mgx; ++g)
				for (int e = 0; e <= (g ? opt->max_gape : 0); ++e) {
					if (a + g + (gape_counts ? e : 0) > mdx + 1) continue;
					const long sc = (long)a * opt->s_mm + (long)g * opt->s_gapo + (long)e * opt->s_gape;
					if (sc + 1 > (long)s.NS1) s.NS1 = (uint32_t)(sc + 1);
				}
		if (s.NS1 > s.NS) s.NS1 = s.NS;
	}
	/* the reference packs the score into 11 bits (bwtgap.c:58) */
	if (s.NS > 2048 || opt->s_mm < 0 || opt->s_gapo < 0 || opt->s_gape < 0 || opt->max_gape < 0 || opt->max_gape > 255)
		return nabwa_fail(NABWA_EINVAL, "option block needs more than 2048 score levels (the reference's own limit)");
	/* first-pass (kernel S) arena entries keep n_mm / n_gapo in 4 bits and n_gape in 5, and it tracks 64 score levels:
	 * option blocks beyond that go to kernel D whole */
	s.deep_only = mdx > 14 || mgx > 15 || opt->max_gape > 31 || s.NS1 > 64;
	if (opt->seed_len < 0) return nabwa_fail(NABWA_EINVAL, "negative seed_len");
	/* refused before any work, not when the first read reaches kernel D in the middle of a file: there a chain's matching child must be
	 * the only child of its own score (fm_deep_body.hpp), so every penalty has to be positive (-M / -O / -E 0 have no use in practice) */
	if (opt->s_mm < 1 || opt->s_gapo < 1 || opt->s_gape < 1) return nabwa_fail(NABWA_EINVAL, "s_mm, s_gapo and s_gape must be >= 1 (-M / -O / -E 0 are not supported)");
	return NABWA_OK;
}

// ---- step 2a, NABWA_DEDUP=1 only: search each distinct read of the batch once.  In: the raw reads of the caller's n_given reads in HBM.
// Out, when some reads are equal in length and in the bytes of both strands: raw_s / raw_r / raw_off hold the n_u distinct reads (the first
// of each set of equal reads, in the caller's order), b->n = n_u, and b->d_map takes each of the caller's reads to the one searched for
// it.  Out, when all reads differ: nothing is changed and no map is kept.
//   hash (dedup_kernels.hip) -> radix sort of (hash, read), stable: a run of equal hashes lists its reads in ascending order -> run
//   starts by an inclusive max-scan -> every read against the first read of its run, byte for byte: equal reads merge, the others (their
//   hashes collided) stay reads of their own, so no result rests on the hash -> exclusive sum of the representatives' flags: their inner
//   indices -> one download (n_u, collisions) -> exclusive sum of their lengths: the compact starts -> their bytes copied.
// bits: how many low bits of the hash the sort sees (NABWA_DEDUP_HASH_BITS, a test knob: with 0 every read lands in one run).
// Everything runs on the batch's stream; the temporaries, about 40 bytes per read beside the compact copy of the reads, are back in the
// pool before the working buffers are taken.
namespace { struct DedupMax { __host__ __device__ uint32_t operator()(uint32_t a, uint32_t c) const { return a > c ? a : c; } }; }

static int dedup_reads(nabwa_batch *b, int bits, PoolBuf<uint8_t> &raw_s, PoolBuf<uint8_t> &raw_r, PoolBuf<int64_t> &raw_off, size_t nb, bool timing)
{
	nabwa_index *ix = b->ix;
	const int n = b->n_given;
	hipStream_t st = b->stream;
	PoolBuf<uint64_t> kA, kB; PoolBuf<uint32_t> vA, vB, head, flag, inner; PoolBuf<int32_t> rep, map; PoolBuf<unsigned int> d_stat;
	PoolBuf<int64_t> coff; PoolBuf<uint8_t> c_s, c_r; PoolBuf<void> d_tmp;
	DevEvent e0, e1;
	StreamDrain drain{ st };
	const size_t n1 = (size_t)n + 1;
	HIP_CHECK(kA.get(ix, n1 * 8)); HIP_CHECK(kB.get(ix, n1 * 8)); HIP_CHECK(vA.get(ix, n1 * 4)); HIP_CHECK(vB.get(ix, n1 * 4));
	HIP_CHECK(head.get(ix, n1 * 4)); HIP_CHECK(rep.get(ix, n1 * 4)); HIP_CHECK(flag.get(ix, n1 * 4)); HIP_CHECK(inner.get(ix, n1 * 4));
	HIP_CHECK(map.get(ix, n1 * 4)); HIP_CHECK(d_stat.get(ix, 8));
	int64_t *const clen = (int64_t*)kA.p;      /* the sort's key buffers are free once the run starts are known: the representatives' lengths go there */
	/* one scratch buffer for the sort and the three scans: the largest of their needs */
	size_t tmp_bytes = 16, need = 0;
	hipcub::DoubleBuffer<uint64_t> dk(kA.p, kB.p); hipcub::DoubleBuffer<uint32_t> dv(vA.p, vB.p);
	HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, need, dk, dv, n, 0, 64, st)); if (need > tmp_bytes) tmp_bytes = need;
	HIP_CHECK(hipcub::DeviceScan::InclusiveScan(nullptr, need, head.p, head.p, DedupMax(), n, st)); if (need > tmp_bytes) tmp_bytes = need;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, flag.p, inner.p, n + 1, st)); if (need > tmp_bytes) tmp_bytes = need;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, clen, clen, n + 1, st)); if (need > tmp_bytes) tmp_bytes = need;
	HIP_CHECK(d_tmp.get(ix, tmp_bytes));
	if (timing) { HIP_CHECK(hipEventCreate(&e0.e)); HIP_CHECK(hipEventCreate(&e1.e)); HIP_CHECK(hipEventRecord(e0, st)); }
	HIP_CHECK(hipMemsetAsync(d_stat, 0, 8, st));
	nabwa_launch_dedup_hash(n, raw_s, raw_r, raw_off, bits >= 64 ? ~0ull : (1ull << bits) - 1ull, kA, vA, st);
	need = tmp_bytes;
	HIP_CHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp.p, need, dk, dv, n, 0, 64, st));
	nabwa_launch_dedup_heads(n, dk.Current(), head, st);
	need = tmp_bytes;
	HIP_CHECK(hipcub::DeviceScan::InclusiveScan(d_tmp.p, need, head.p, head.p, DedupMax(), n, st));
	nabwa_launch_dedup_verify(n, raw_s, raw_r, raw_off, dv.Current(), head, rep, flag, d_stat, st);
	need = tmp_bytes;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, need, flag.p, inner.p, n + 1, st));
	nabwa_launch_dedup_map(n, rep, inner, raw_off, map, clen, d_stat, st);
	unsigned int stat[2] = { 0, 0 };      /* collisions, distinct reads */
	HIP_CHECK(hipMemcpyAsync(stat, d_stat, 8, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	HIP_CHECK(hipGetLastError());
	const int n_u = (int)stat[1];
	if (n_u < 1 || n_u > n) return nabwa_fail(NABWA_EIO, "NABWA_DEDUP: the stage counted more distinct reads than reads, or none");
	b->dedup_coll = stat[0];
	if (n_u < n) {
		HIP_CHECK(coff.get(ix, ((size_t)n_u + 1) * 8)); HIP_CHECK(c_s.get(ix, nb)); HIP_CHECK(c_r.get(ix, nb));
		need = tmp_bytes;
		HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, need, clen, coff.p, n_u + 1, st));
		nabwa_launch_dedup_compact(n, raw_s, raw_r, raw_off, rep, inner, coff, c_s, c_r, st);
	}
	if (timing) HIP_CHECK(hipEventRecord(e1, st));
	HIP_CHECK(hipStreamSynchronize(st));
	HIP_CHECK(hipGetLastError());
	if (timing) {
		float ms = 0.f;
		HIP_CHECK(hipEventElapsedTime(&ms, e0, e1));
		fprintf(stderr, "[nabwa] dedup: %d reads given, %d searched, %u hash collisions, stage %.3f ms\n", n, n_u, stat[0], ms);
	}
	if (n_u < n) {      /* (the stream is idle: the buffers these replace go back to the pool) */
		raw_s = std::move(c_s); raw_r = std::move(c_r); raw_off = std::move(coff);
		b->d_map = std::move(map);
		b->n = n_u;
	}
	return NABWA_OK;
}

// ---- step 2b, NABWA_DEDUP_CACHE only: the distinct reads that an earlier batch on this index searched under the same options are served from
// the index's read cache.  In: raw_s / raw_r / raw_off hold the b->n pairwise distinct reads dedup_reads left, b->d_map (or
// none) takes the caller's reads to them.  Out, when n_served > 0 of them were found: the raw buffers hold the others, in order, b->n is
// their number (0: nothing is left to search), b->d_cent names the entries and b->d_map takes a caller's read to a read searched (>= 0) or to
// served read -1 - value; the cache is pinned.  Out, when none was found: nothing is changed.
//   the option signature decides first: the cache's -> use it; another and no live batch holds references -> empty the cache (a flush), then
//   use it; another and references are held -> this batch goes without the cache (a bypass)
//   hash of every read (all 64 bits) -> probe and compare (dedup_cache_kernels.hip) -> exclusive sum of the flags of the reads to search ->
//   their numbers and lengths, the served reads' entries -> one download (reads to search) -> compact starts -> their bytes; the map
// The cache's mutex is held from the first launch until the stream is idle.
static uint64_t option_signature(const nabwa_gap_opt_t *o)
{
	uint32_t fnr; memcpy(&fnr, &o->fnr, 4);
	const uint32_t w[14] = { (uint32_t)o->s_mm, (uint32_t)o->s_gapo, (uint32_t)o->s_gape, (uint32_t)o->mode, (uint32_t)o->indel_end_skip, (uint32_t)o->max_del_occ,
							 (uint32_t)o->max_entries, fnr, (uint32_t)o->max_diff, (uint32_t)o->max_gapo, (uint32_t)o->max_gape, (uint32_t)o->max_seed_diff,
							 (uint32_t)o->seed_len, (uint32_t)o->max_top2 };      /* every field that reaches the search: not n_threads, not trim_qual (the reads come trimmed) */
	uint64_t h = 0xcbf29ce484222325ULL;
	for (uint32_t x : w) for (int k = 0; k < 4; ++k) { h ^= (x >> (8 * k)) & 0xffu; h *= 0x100000001b3ULL; }
	return h;
}

static int cache_lookup(nabwa_batch *b, const BatchShape &s, PoolBuf<uint8_t> &raw_s, PoolBuf<uint8_t> &raw_r, PoolBuf<int64_t> &raw_off, size_t nb, bool timing)
{
	nabwa_index *ix = b->ix;
	nabwa_dedup_cache *c = b->cache;
	const int n = b->n, max_len = s.max_len;
	hipStream_t st = b->stream;
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->has_sig && c->sig != b->cache_sig) {
		if (c->pins) { ++c->bypasses; b->cache = nullptr; b->cache_bypass = 1; return NABWA_OK; }
		if (int r = nabwa_dcache_reset(ix, c)) return r;
		++c->flushes;
	}
	c->sig = b->cache_sig; c->has_sig = true;
	PoolBuf<uint64_t> hash; PoolBuf<uint32_t> ids, found, flag, inner, cent; PoolBuf<int32_t> rep, newidx, map; PoolBuf<int64_t> clen, coff; PoolBuf<unsigned int> d_stat;
	PoolBuf<uint8_t> d_tab, c_s, c_r; PoolBuf<void> d_tmp;
	DevEvent e0, e1;
	StreamDrain drain{ st };
	const size_t n1 = (size_t)n + 1;
	HIP_CHECK(hash.get(ix, n1 * 8)); HIP_CHECK(ids.get(ix, n1 * 4)); HIP_CHECK(found.get(ix, n1 * 4)); HIP_CHECK(flag.get(ix, n1 * 4)); HIP_CHECK(inner.get(ix, n1 * 4));
	HIP_CHECK(cent.get(ix, n1 * 4)); HIP_CHECK(rep.get(ix, n1 * 4)); HIP_CHECK(newidx.get(ix, n1 * 4)); HIP_CHECK(clen.get(ix, n1 * 8)); HIP_CHECK(d_stat.get(ix, 8));
	HIP_CHECK(d_tab.get(ix, 2 * (size_t)(max_len + 1)));
	size_t tmp_bytes = 16, need = 0;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, flag.p, inner.p, n + 1, st)); if (need > tmp_bytes) tmp_bytes = need;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, need, clen.p, clen.p, n + 1, st)); if (need > tmp_bytes) tmp_bytes = need;
	HIP_CHECK(d_tmp.get(ix, tmp_bytes));
	HIP_CHECK(hipEventCreate(&e0.e)); HIP_CHECK(hipEventCreate(&e1.e)); HIP_CHECK(hipEventRecord(e0, st));
	HIP_CHECK(hipMemcpyAsync(d_tab, s.md_tab.data(), max_len + 1, hipMemcpyHostToDevice, st));
	HIP_CHECK(hipMemcpyAsync(d_tab + max_len + 1, s.mg_tab.data(), max_len + 1, hipMemcpyHostToDevice, st));
	nabwa_launch_dedup_hash(n, raw_s, raw_r, raw_off, ~0ull, hash, ids, st);
	nabwa_launch_dcache_lookup(n, raw_s, raw_r, raw_off, hash, d_tab, d_tab + max_len + 1, c->d_slots, c->n_slots, b->cache_mask, c->d_arena, found, flag, st);
	need = tmp_bytes;
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, need, flag.p, inner.p, n + 1, st));
	nabwa_launch_dcache_map(n, found, inner, raw_off, rep, newidx, clen, cent, d_stat, st);
	unsigned int n_search = 0;
	HIP_CHECK(hipMemcpyAsync(&n_search, d_stat, 4, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipStreamSynchronize(st));
	HIP_CHECK(hipGetLastError());
	if ((int)n_search < 0 || (int)n_search > n) return nabwa_fail(NABWA_EIO, "NABWA_DEDUP_CACHE: the lookup counted more reads to search than reads");
	const int n_s = (int)n_search, n_served = n - n_s;
	c->lookups += (uint64_t)n; c->served += (uint64_t)n_served;
	if (n_served) {
		HIP_CHECK(coff.get(ix, ((size_t)n_s + 1) * 8)); HIP_CHECK(c_s.get(ix, nb)); HIP_CHECK(c_r.get(ix, nb)); HIP_CHECK(map.get(ix, (size_t)b->n_given * 4));
		if (n_s) {
			need = tmp_bytes;
			HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, need, clen.p, coff.p, n_s + 1, st));
			nabwa_launch_dedup_compact(n, raw_s, raw_r, raw_off, rep, inner, coff, c_s, c_r, st);
		} else HIP_CHECK(hipMemsetAsync(coff, 0, 8, st));
		nabwa_launch_dcache_remap(b->n_given, b->d_map, newidx, map, st);
	}
	HIP_CHECK(hipEventRecord(e1, st));
	HIP_CHECK(hipStreamSynchronize(st));
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventElapsedTime(&b->cache_lookup_ms, e0, e1));
	if (timing) fprintf(stderr, "[nabwa] dedup cache: %d reads looked up, %d to search, %d served, stage %.3f ms\n", n, n_s, n_served, b->cache_lookup_ms);
	if (n_served) {      /* (the stream is idle: the buffers these replace go back to the pool) */
		raw_s = std::move(c_s); raw_r = std::move(c_r); raw_off = std::move(coff);
		b->d_map = std::move(map); b->d_cent = std::move(cent);
		b->n = n_s; b->n_served = n_served;
		++c->pins; b->cache_pinned = 1;
	}
	return NABWA_OK;
}

// ---- step 2: the reads, uploaded as given, then re-laid out on the device with 16-byte aligned starts
// dedup_bits: -1, or with NABWA_DEDUP=1 the hash bits of dedup_reads, which then runs between the upload and the re-layout
static int upload_reads(nabwa_batch *b, const BatchShape &s, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, bool timing, double tc0, int dedup_bits)
{
	nabwa_index *ix = b->ix;
	const int n_given = b->n_given, max_len = s.max_len;
	const size_t nb = (size_t)off[n_given] > 0 ? (size_t)off[n_given] : 1, pnb = (size_t)s.padded_total + 64;
	if ((uint64_t)pnb >= (1ull << 32)) return nabwa_fail(NABWA_EINVAL, "batch holds 4 Gi padded bases or more: split it (lane state keeps a 32-bit read offset)");
	/* the batch's read buffers, for n reads; with NABWA_DEDUP=1 they are taken once the distinct reads are counted (d_seq / d_rseq keep the
	 * caller's padded total, which the host knows; the distinct reads need no more) */
	auto read_buffers = [&](int n) -> int {
		HIP_CHECK(b->d_seq.get(ix, pnb)); HIP_CHECK(b->d_rseq.get(ix, pnb));
		HIP_CHECK(b->d_poff.get(ix, (size_t)(n + 1) * 8)); HIP_CHECK(b->d_len.get(ix, (size_t)(n ? n : 1) * 4));
		HIP_CHECK(b->d_md.get(ix, n ? n : 1)); HIP_CHECK(b->d_mg.get(ix, n ? n : 1)); HIP_CHECK(b->d_key.get(ix, (size_t)(n ? n : 1) * 24));
		b->pack_stride = 2 * ((max_len + 15) / 16 + 2);
		HIP_CHECK(b->d_pack.get(ix, (size_t)(n ? n : 1) * b->pack_stride * 4));
		HIP_CHECK(b->d_cls.get(ix, (size_t)(n ? n : 1) * 2)); HIP_CHECK(b->d_perm.get(ix, (size_t)(n ? n : 1) * 4)); HIP_CHECK(b->d_ncls.get(ix, NCLS_WORDS * sizeof(unsigned int)));
		return NABWA_OK;
	};
	const bool dedup = dedup_bits >= 0 && n_given > 0;
	if (!dedup) if (int r = read_buffers(n_given)) return r;
	if (n_given == 0) { HIP_CHECK(hipMemset(b->d_poff, 0, 8)); return NABWA_OK; }
	PoolBuf<uint8_t> raw_s, raw_r, d_tab; PoolBuf<int64_t> raw_off, plen; PoolBuf<void> d_tmp; size_t tmp_bytes = 0;
	StreamDrain drain{ b->stream };
	HIP_CHECK(raw_s.get(ix, nb)); HIP_CHECK(raw_r.get(ix, nb)); HIP_CHECK(raw_off.get(ix, (size_t)(n_given + 1) * 8));
	const UploadJob jobs[3] = { { raw_s, seq, (size_t)off[n_given] }, { raw_r, rseq, (size_t)off[n_given] }, { raw_off, off, (size_t)(n_given + 1) * 8 } };
	const double tu0 = now_s();
	HIP_CHECK(staged_upload(ix, jobs, 3));
	if (timing) fprintf(stderr, "[nabwa] upload of %.2f GB: %.3f s (%.3f s into batch_create)\n", 2e-9 * (double)off[n_given], now_s() - tu0, tu0 - tc0);
	if (dedup) {
		if (int r = dedup_reads(b, dedup_bits, raw_s, raw_r, raw_off, nb, timing)) return r;
		if (b->cache) if (int r = cache_lookup(b, s, raw_s, raw_r, raw_off, nb, timing)) return r;
		if (int r = read_buffers(b->n)) return r;
	}
	const int n = b->n;      /* the reads searched from here on */
	// padded starts: exclusive scan of the padded lengths, on the device
	HIP_CHECK(plen.get(ix, (size_t)(n + 1) * 8));
	nabwa_launch_padded_len(n, raw_off, plen, b->stream);
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, plen.p, b->d_poff.p, n + 1, b->stream));
	HIP_CHECK(d_tmp.get(ix, tmp_bytes ? tmp_bytes : 16));
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, plen.p, b->d_poff.p, n + 1, b->stream));
	HIP_CHECK(d_tab.get(ix, 2 * (size_t)(max_len + 1)));
	HIP_CHECK(hipMemcpyAsync(d_tab, s.md_tab.data(), max_len + 1, hipMemcpyHostToDevice, b->stream));
	HIP_CHECK(hipMemcpyAsync(d_tab + max_len + 1, s.mg_tab.data(), max_len + 1, hipMemcpyHostToDevice, b->stream));
	nabwa_launch_pad_reads(n, raw_s, raw_r, raw_off, b->d_poff, b->d_seq, b->d_rseq, b->d_len, b->d_key,
						   ix->bwt[0].kmer_T == ix->bwt[1].kmer_T ? (int)ix->bwt[0].kmer_T : 0, b->opt.seed_len, b->d_pack, b->pack_stride,
						   d_tab, d_tab + max_len + 1, b->d_md, b->d_mg, b->stream);
	HIP_CHECK(hipStreamSynchronize(b->stream));
	if (timing) fprintf(stderr, "[nabwa] re-layout kernel done %.3f s into batch_create\n", now_s() - tc0);
	HIP_CHECK(raw_s.release()); HIP_CHECK(raw_r.release()); HIP_CHECK(raw_off.release());
	HIP_CHECK(plen.release()); HIP_CHECK(d_tmp.release()); HIP_CHECK(d_tab.release());
	return NABWA_OK;
}

// ---- step 3: the search parameters, the launch shape and the working buffers
static int working_buffers(nabwa_batch *b, const BatchShape &s)
{
	nabwa_index *ix = b->ix;
	const nabwa_gap_opt_t *opt = &b->opt;
	const int n = b->n, max_len = s.max_len;
	SearchParams &P = b->P;
	memset(&P, 0, sizeof(P));
	P.bwt[0] = ix->bwt[0]; P.bwt[1] = ix->bwt[1];
	{	/* the per-index constants the search kernels pick per lane, as a table for their LDS (fm_search.hpp) */
		uint32_t tab[NABWA_IXTAB_ALL];
		nabwa_ixtab_fill(tab, ix->bwt);
		memcpy(tab + NABWA_IXTAB_WORDS, ix->kmer_pk, sizeof ix->kmer_pk);      /* kernel W's primary keys, behind kernel D's words */
		HIP_CHECK(b->d_ixtab.get(ix, sizeof tab));
		HIP_CHECK(hipMemcpy(b->d_ixtab, tab, sizeof tab, hipMemcpyHostToDevice));
		P.ixtab = b->d_ixtab;
	}
	P.seq = b->d_seq; P.rseq = b->d_rseq; P.poff = b->d_poff; P.rd_len = b->d_len; P.rd_maxdiff = b->d_md; P.rd_maxgapo = b->d_mg; P.rd_key = b->d_key; P.rd_pack = b->d_pack; P.pack_stride = b->pack_stride;
	P.text_mode = env_int("NABWA_TEXT_KERNELS", 7) & 7;      /* bit 0: text mode in the width kernel, bit 1: in the search kernel, bit 2: key form in the search kernel */
	/* kernel W (fm_search.hip; profiles/width_requests_bench.txt): NABWA_W_QUADS -- a table trip takes two levels from each 32 bytes it loads, the
	 * parent's width as the sum over its children (0: one 8-byte entry per level, as before v14) */
	if (env_int("NABWA_W_QUADS", 1)) P.text_mode |= TM_W_QUADS;
	/* (profiles/width_spans_bench.txt) NABWA_W_RUNS -- text runs of up to 16 positions from any position of either pass; NABWA_W_TRIP8 -- table trips
	 * of up to 8 levels that may end a pass; the outputs of either are appended to the record's accumulators as values, in one shift and merge.
	 * Both 0: the kernel before v15 */
	if (env_int("NABWA_W_RUNS", 1)) P.text_mode |= TM_W_RUNS;
	if (env_int("NABWA_W_TRIP8", 1)) P.text_mode |= TM_W_TRIP8;
	if (ix->bwt[0].kmer_T != ix->bwt[1].kmer_T) P.bwt[0].kmer_T = P.bwt[1].kmer_T = 0;
	P.ids = 0; P.n = n;
	P.s_mm = opt->s_mm; P.s_gapo = opt->s_gapo; P.s_gape = opt->s_gape; P.mode = opt->mode;
	P.indel_end_skip = opt->indel_end_skip; P.max_del_occ = opt->max_del_occ; P.max_entries = opt->max_entries;
	P.max_gape = opt->max_gape; P.max_seed_diff = opt->max_seed_diff; P.seed_len = opt->seed_len; P.max_top2 = opt->max_top2;
	int cap1 = env_int("NABWA_CAP1", 4096);
	if (cap1 < 16) cap1 = 16;
	if (cap1 > 65534) cap1 = 65534;
	layout(P, (uint32_t)cap1, max_len, opt->seed_len, s.deep_only ? 1u : s.NS1);
	P.aln_cap = env_int("NABWA_ALNCAP1", 16);
	P.sync_refill = env_int("NABWA_SYNC_REFILL", 0);
	/* trips after which kernel S hands a search on to kernel D (0: never).  Seeded searches (the default options): measured 10 M x 100 bp,
	 * 0 -> 123.6 ms per pass, 2000 -> 108.9 (1111 reads handed on, kernel D 2 ms), 1000 -> 116.2, 500 -> 189.6; 2 x 150 bp pairs: 2000 is the
	 * optimum too.  Without a seed (reads no longer than seed_len: the ancient-DNA options) the searches that do not end early are deep, and
	 * every trip kernel S spends on them is spent again by kernel D: 6.25 M reads, 300 / 1000 / 2000 / 5000 -> 2.29 / 2.20 / 2.20 / 2.04 M reads/s */
	P.trip_budget = (uint32_t)env_int("NABWA_TRIP_BUDGET", max_len > opt->seed_len ? 2000 : 300);
	P.trip_budget_hard = (uint32_t)env_int("NABWA_TRIP_BUDGET_HARD", max_len > opt->seed_len ? 200 : (int)P.trip_budget);      /* (a batch of reads that mostly occur on neither strand: fm_search.hip) */
	if (getenv("NABWA_TRIP_BUDGET") && !getenv("NABWA_TRIP_BUDGET_HARD")) P.trip_budget_hard = P.trip_budget;                       /* (a sweep of the one knob means the one budget) */
	b->class_sort = env_int("NABWA_CLASS_SORT", 1);
	/* kernel S's shortcut for a read one of whose strands occurs exactly (kernel W's class 0; fm_search.hip): 0 off, 1 nothing stored that
	 * cannot be popped + 1-mismatch key-form children resolved where they are created, 2 also the surviving ones stored landed, 3 also the leap: a
	 * text-form entry that is the read's own prefix on a strand that occurs is replaced by its hit (profiles/exact_leap_bench.txt) */
	P.sure0 = env_int("NABWA_SURE0", 3);
	if (P.sure0 < 0) P.sure0 = 0;
	if (P.sure0 > 3) P.sure0 = 3;
	if (env_int("NABWA_SURE0_STATS", 0)) {
		HIP_CHECK(b->d_s0stats.get(ix, S0S_WORDS * sizeof(unsigned long long)));
		HIP_CHECK(hipMemset(b->d_s0stats, 0, S0S_WORDS * sizeof(unsigned long long)));
		P.s0_stats = b->d_s0stats;
	}
	{
		P.w_sync = (n > 0 && s.min_len == max_len) ? env_int("NABWA_W_SYNC", 1) : 0;
	}
	if (P.aln_cap < 1) P.aln_cap = 1;

	hipDeviceProp_t prop;
	HIP_CHECK(hipGetDeviceProperties(&prop, ix->device));
	int occ = nabwa_search_occupancy(s.deep_only ? 1 : (int)s.NS1);
	if (occ < 1) occ = 1;
	const int occ_env = env_int("NABWA_BLOCKS_PER_CU", 0);
	if (occ_env > 0) occ = occ_env;
	long blocks = (long)prop.multiProcessorCount * occ;
	const long need = ((long)n + NABWA_SEARCH_BLOCK - 1) / NABWA_SEARCH_BLOCK;
	if (blocks > need) blocks = need;
	if (blocks < 1) blocks = 1;
	b->n_blocks = (int)blocks;
	if (getenv("NABWA_TIMING")) fprintf(stderr, "[nabwa] search kernel: %u score levels, %d blocks per CU (LDS %zu B per block), %ld blocks\n", s.NS1, occ,
										(size_t)s.NS1 * NABWA_SEARCH_BLOCK * 2 + NABWA_SEARCH_BLOCK * 80, blocks);
	HIP_CHECK(b->d_scratch.get(ix, (size_t)blocks * NABWA_SEARCH_BLOCK * P.lane_stride));
	int occw = nabwa_width_occupancy(P.text_mode); if (occw < 1) occw = 1;
	long blocks_w = (long)prop.multiProcessorCount * occw;
	if (blocks_w > 2 * need) blocks_w = 2 * need;        /* kernel W: one lane per strand of a read */
	if (blocks_w < 1) blocks_w = 1;
	b->n_blocks_w = (int)blocks_w;
	HIP_CHECK(b->d_wdata.get(ix, (size_t)(n ? n : 1) * P.wstride));
	HIP_CHECK(b->d_nN.get(ix, n ? n : 1));
	P.wdata = b->d_wdata; P.rd_nN = b->d_nN;
	const size_t n1 = n ? n : 1;
	HIP_CHECK(b->d_naln.get(ix, n1 * 4)); HIP_CHECK(b->d_maxent.get(ix, n1 * 4)); HIP_CHECK(b->d_wide_idx.get(ix, n1 * 4));
	HIP_CHECK(b->d_status.get(ix, n1)); HIP_CHECK(b->d_aln.get(ix, n1 * (size_t)P.aln_cap * 16));
	HIP_CHECK(b->d_counter.get(ix, WC_WORDS * sizeof(unsigned int))); HIP_CHECK(b->d_novf.get(ix, 4)); HIP_CHECK(b->d_ovf_ids.get(ix, n1 * 4));
	HIP_CHECK(b->d_sum.get(ix, TS_WORDS * sizeof(unsigned long long)));
	P.scratch = b->d_scratch; P.n_aln = b->d_naln; P.max_ent = b->d_maxent; P.status = b->d_status; P.aln = b->d_aln;
	P.work_counter = b->d_counter;
	return NABWA_OK;
}

extern "C" int nabwa_batch_create(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off,
								  const uint8_t *seq, const uint8_t *rseq, int per_read, nabwa_batch_t **out)
{
	if (!ix || !opt || !off || !out || n < 0 || (n && (!seq || !rseq))) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(ix->device));
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double tc0 = now_s();
	/* NABWA_DEDUP: unset or 0 -- every read is searched; 1 -- each distinct read once (dedup_reads).  NABWA_DEDUP_HASH_BITS (tests): the low
	 * bits of the hash that group the reads, 0..64 */
	int dedup_bits = -1;
	if (const char *e = getenv("NABWA_DEDUP")) {
		if (strcmp(e, "0") && strcmp(e, "1")) return nabwa_fail(NABWA_EINVAL, "NABWA_DEDUP: 0 or 1");
		if (e[0] == '1') {
			dedup_bits = 64;
			if (const char *k = getenv("NABWA_DEDUP_HASH_BITS")) {
				char *end = 0;
				const long v = strtol(k, &end, 10);
				if (end == k || *end || v < 0 || v > 64) return nabwa_fail(NABWA_EINVAL, "NABWA_DEDUP_HASH_BITS: 0..64");
				dedup_bits = (int)v;
			}
		}
	}
	/* NABWA_DEDUP_CACHE: unset or 0 -- no batch remembers another's reads; a number of MiB -- the distinct reads NABWA_DEDUP=1 leaves are looked up
	 * in the index's read cache before the search and entered into it after (cache_lookup, cache_insert); the first batch to ask makes the cache */
	nabwa_dedup_cache *cache = nullptr;
	if (const char *e = getenv("NABWA_DEDUP_CACHE")) {
		char *end = 0;
		const long v = strtol(e, &end, 10);
		if (end == e || *end || v < 0) return nabwa_fail(NABWA_EINVAL, "NABWA_DEDUP_CACHE: a number of MiB, 0 for off");
		if (v > 0 && dedup_bits < 0) return nabwa_fail(NABWA_EINVAL, "NABWA_DEDUP_CACHE needs NABWA_DEDUP=1: the cache sits behind the in-batch stage");
		if (v > 0) if (int r = nabwa_dcache_get(ix, v, &cache)) return r;
	}
	BatchShape s;
	if (int r = derive_options(opt, n, off, per_read, s)) return r;      /* (on the caller's reads, whatever NABWA_DEDUP says: the lengths that occur are the same) */

	const double tc1 = now_s();
	std::unique_ptr<nabwa_batch, void (*)(nabwa_batch*)> b(new nabwa_batch(), nabwa_batch_destroy);      /* a half-built batch goes the way of a whole one */
	b->ix = ix; b->opt = *opt; b->n = b->n_given = n; b->dedup_on = dedup_bits >= 0; b->deep_only = s.deep_only ? 1 : 0;
	b->max_len = s.max_len; b->min_len = n ? s.min_len : 0; b->NS1 = s.NS1; b->NS_wide = s.NS; b->deep_coop = -1;
	if (cache) { b->cache = cache; b->cache_on = 1; b->cache_sig = option_signature(opt); b->cache_mask = dedup_bits >= 64 ? ~0ull : (1ull << dedup_bits) - 1ull; }
	/* a stream that does not synchronise with the legacy default stream: the finishing chains of another batch (bwt_sa batches, the
	 * alignment kernels: default stream, synchronous copies) run from another thread while this batch's search kernels do; everything in
	 * this file orders its own work on b->stream explicitly.  NABWA_STREAM_BLOCKING=1: the old kind, for comparison. */
	if (env_int("NABWA_STREAM_BLOCKING", 0)) HIP_CHECK(hipStreamCreate(&b->stream.s));
	else HIP_CHECK(hipStreamCreateWithFlags(&b->stream.s, hipStreamNonBlocking));
	for (DevEvent *e : { &b->ev0, &b->ev1, &b->evw, &b->evd0, &b->evd1 }) HIP_CHECK(hipEventCreate(&e->e));
	if (int r = upload_reads(b.get(), s, off, seq, rseq, timing, tc0, dedup_bits)) return r;

	const double tc2 = now_s();
	if (int r = working_buffers(b.get(), s)) return r;
	*out = b.release();
	if (timing) fprintf(stderr, "[nabwa] batch_create %d reads: host option derivation %.3f s, read upload + device layout %.3f s, working buffers %.3f s\n", n, tc1 - tc0, tc2 - tc1, now_s() - tc2);
	return NABWA_OK;
}

/* NABWA_W_STATS=1: this launch of kernel W is its statistics instantiation (fm_search.hip: with tables, unlike the counting run); its counts, slots
 * TS_W_* of d_sum, are read and printed at the next synchronisation of the stream */
static int w_stats_arm(nabwa_batch *b, SearchParams &PW)
{
	if (!env_int("NABWA_W_STATS", 0) || PW.touch_counter) return NABWA_OK;
	HIP_CHECK(hipMemsetAsync(b->d_sum + TS_W_TRIPS, 0, 6 * sizeof(unsigned long long), b->stream));
	PW.touch_counter = b->d_sum; PW.text_mode |= TM_W_STATS; b->w_stats_armed = 1;
	return NABWA_OK;
}
static int w_stats_collect(nabwa_batch *b)
{
	if (!b->w_stats_armed) return NABWA_OK;
	b->w_stats_armed = 0;
	unsigned long long *t = b->w_stats;
	HIP_CHECK(hipMemcpy(t, b->d_sum + TS_W_TRIPS, 6 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
	const unsigned long long lo = 0xffffffffull;
	fprintf(stderr, "[nabwa] width kernel: wave-trips %llu; lane-trips / positions: text %llu / %llu (in seed passes: %llu trips), table %llu / %llu, step with a rank query %llu, step without %llu; longest item %llu trips\n",
			t[0], t[2] >> 32, t[2] & lo, t[4] >> 32, t[3] >> 32, t[3] & lo, t[4] & lo, t[5], t[1]);
	return NABWA_OK;
}
/* Tests and profiles: the six words TS_W_TRIPS .. TS_W_STEP (search_slots.hpp) of the last launch of kernel W that ran with NABWA_W_STATS=1 */
extern "C" int nabwa_batch_w_stats(nabwa_batch_t *b, unsigned long long *out)
{
	if (!b || !out) return nabwa_fail(NABWA_EINVAL, "bad argument");
	memcpy(out, b->w_stats, sizeof b->w_stats);
	return NABWA_OK;
}

extern "C" int nabwa_batch_run(nabwa_batch_t *b)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null batch");
	HIP_CHECK(hipSetDevice(b->ix->device));
	b->unresolved = 0;
	if (b->n == 0) return NABWA_OK;
	if (b->n_grown) {          /* row blocks of the previous run's longest hit lists: that run's results are gone with this one */
		HIP_CHECK(hipStreamSynchronize(b->stream));
		for (int t = 0; t < b->n_grown; ++t) HIP_CHECK(b->grown[t].release());
		b->n_grown = 0; b->grown_used = 0;
	}
	HIP_CHECK(hipMemsetAsync(b->d_counter, 0, WC_WORDS * sizeof(unsigned int), b->stream));
	HIP_CHECK(hipMemsetAsync(b->d_novf, 0, 4, b->stream));
	HIP_CHECK(hipEventRecord(b->evw, b->stream));
	SearchParams PW = b->P; PW.ids = 0; PW.rd_cls = b->class_sort ? b->d_cls : 0;
	if (int r = w_stats_arm(b, PW)) return r;
	nabwa_launch_fm_width(&PW, b->n_blocks_w, b->stream);
	if (b->class_sort) {      /* work order of the search: reads with an exact occurrence first, in lockstep waves */
		HIP_CHECK(hipMemsetAsync(b->d_ncls, 0, NCLS_WORDS * sizeof(unsigned int), b->stream));
		nabwa_launch_partition(b->n, b->d_cls, b->d_perm, b->d_ncls, b->stream);
	}
	HIP_CHECK(hipEventRecord(b->ev0, b->stream));
	SearchParams PS = b->P; PS.ids = b->class_sort ? b->d_perm : 0; PS.n_sync = b->class_sort ? b->d_ncls + NCLS_FIRST0 : 0;
	PS.rd_cls = b->class_sort ? b->d_cls : 0;      /* (this launch only: the re-runs over handed-on reads search without the shortcut) */
	if (!b->deep_only) nabwa_launch_fm_search(&PS, b->n_blocks, b->stream);
	else {      /* option blocks the first-pass kernel's compact entries cannot hold: every read goes to kernel D */
		HIP_CHECK(hipMemsetAsync(b->d_status, NABWA_ST_OVERFLOW, b->n, b->stream));
		HIP_CHECK(hipMemsetAsync(b->d_naln, 0, (size_t)b->n * 4, b->stream));
	}
	HIP_CHECK(hipEventRecord(b->ev1, b->stream));
	/* the reads the first pass hands on, in the order kernel D should start them (largest-looking searches first) */
	if (b->class_sort && env_int("NABWA_DEEP_ORDER", 1)) nabwa_launch_collect_keyed(b->n, b->d_status, b->d_ovf_ids, b->d_novf, NABWA_ST_OVERFLOW, b->d_cls, b->d_md, 7, b->d_naln, b->P.aln_cap, b->stream);
	else nabwa_launch_collect(b->n, b->d_status, b->d_ovf_ids, b->d_novf, NABWA_ST_OVERFLOW, b->stream);
	HIP_CHECK(hipGetLastError());
	b->ran = 1;
	return NABWA_OK;
}

/* ---- nabwa_batch_sync: the reads kernel S flagged go to kernel D (nabwa_batch_deep.hip).  Optionally the first-pass kernel runs once
 * more before that with the largest arena its 16-bit links address (NABWA_TIER_A=1). */

// the kernel-W records of the listed reads again: a search edits them in place (gap_shadow)
void rebuild_widths(nabwa_batch *b, const SearchParams &Q, unsigned int cnt, bool after_first_pass)
{
	SearchParams QW = Q; QW.touch_counter = 0; QW.rd_cls = 0; QW.n_sync = 0; QW.w_sync = 0;
	/* only a search that found a hit has edited its record; after kernel D has had a read (the guaranteed pass, the searches with longer
	 * hit lists) its record is rebuilt whatever it found */
	QW.w_skip_clean = after_first_pass && env_int("NABWA_W_SKIP_CLEAN", 1) ? 1 : 0;
	QW.n_aln = b->d_naln; QW.max_ent = b->d_maxent; QW.status = b->d_status; QW.aln = b->d_aln; QW.aln_cap = b->P.aln_cap;
	long bw2 = (2 * (long)cnt + NABWA_SEARCH_BLOCK - 1) / NABWA_SEARCH_BLOCK;     /* one lane per strand */
	if (bw2 > b->n_blocks_w) bw2 = b->n_blocks_w;
	(void)hipMemsetAsync(b->d_counter, 0, WC_WORDS * sizeof(unsigned int), b->stream);       /* kernel W draws its work items from WC_WIDTH */
	nabwa_launch_fm_width(&QW, (int)bw2, b->stream);
}

/* the reads of status `which` into d_ovf_ids, their number into *left; the stream is idle afterwards */
int recollect(nabwa_batch *b, int which, unsigned int *left)
{
	HIP_CHECK(hipMemsetAsync(b->d_novf, 0, 4, b->stream));
	nabwa_launch_collect(b->n, b->d_status, b->d_ovf_ids, b->d_novf, which, b->stream);
	HIP_CHECK(hipMemcpyAsync(left, b->d_novf, 4, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipStreamSynchronize(b->stream));
	return NABWA_OK;
}

/* NABWA_TIER_A=1: the first-pass kernel once more over the *cur listed reads, with the largest arena its 16-bit links address */
static int tier_a_rerun(nabwa_batch *b, unsigned int *cur, bool timing)
{
	const double tt0 = now_s();
	SearchParams Q = b->P;
	layout(Q, 65534u, b->max_len, b->opt.seed_len, b->P.NS);
	long blocks = ((long)*cur + NABWA_SEARCH_BLOCK - 1) / NABWA_SEARCH_BLOCK;
	size_t budget = (size_t)env_int("NABWA_WIDE_GB", 32) << 30;
	const long fit = (long)(budget / ((size_t)NABWA_SEARCH_BLOCK * Q.lane_stride));
	if (blocks > fit) blocks = fit < 1 ? 1 : fit;
	const size_t need = (size_t)blocks * NABWA_SEARCH_BLOCK * Q.lane_stride;
	if (b->scratch2_bytes < need) {
		b->scratch2_bytes = 0;
		HIP_CHECK(b->d_scratch2.release());
		HIP_CHECK(b->d_scratch2.get(b->ix, need));
		b->scratch2_bytes = need;
	}
	Q.scratch = b->d_scratch2; Q.ids = b->d_ovf_ids; Q.n = (int)*cur; Q.n_sync = 0; Q.w_sync = 0;
	rebuild_widths(b, Q, *cur, false);
	HIP_CHECK(hipMemsetAsync(b->d_counter, 0, WC_WORDS * sizeof(unsigned int), b->stream));
	nabwa_launch_fm_search(&Q, (int)blocks, b->stream);
	HIP_CHECK(hipGetLastError());
	unsigned int left = 0;
	if (int r = recollect(b, NABWA_ST_OVERFLOW, &left)) return r;
	if (timing) fprintf(stderr, "[nabwa] first-pass kernel again, arena of 65534 entries: %u reads on %ld blocks, %u left, %.3f s\n", *cur, blocks, left, now_s() - tt0);
	*cur = left;
	return NABWA_OK;
}

/* NABWA_DEDUP_CACHE: the reads this batch searched, their results final, into the index's read cache -- once per batch, however often it runs.
 * A read enters when its search is complete, it has at most row_cap rows (NABWA_DEDUP_CACHE_ROWS, default 1024 -- the default capacity of
 * the wide rows: an entry stays within 16 KiB of rows --, never below the narrow row capacity NABWA_ALNCAP1), a slot of its chain is free within the probe bound and the arena has room (dedup_cache_kernels.hip).  A cache that
 * was emptied for another option block since this batch looked up takes nothing from it.  The cache's mutex is held until the stream is idle. */
static int cache_insert(nabwa_batch *b)
{
	nabwa_dedup_cache *c = b->cache;
	hipStream_t st = b->stream;
	std::lock_guard<std::mutex> lk(c->mu);
	b->cache_inserted = 1;
	if (!c->has_sig) { c->sig = b->cache_sig; c->has_sig = true; }      /* (cleared since the lookup) */
	if (c->sig != b->cache_sig) { b->n_not_inserted = (uint64_t)b->n; return NABWA_OK; }
	int row_cap = env_int("NABWA_DEDUP_CACHE_ROWS", 1024);
	if (row_cap < b->P.aln_cap) row_cap = b->P.aln_cap;
	unsigned long long c0[DC_WORDS], c1[DC_WORDS];
	DevEvent e0, e1;
	StreamDrain drain{ st };
	HIP_CHECK(hipEventCreate(&e0.e)); HIP_CHECK(hipEventCreate(&e1.e)); HIP_CHECK(hipEventRecord(e0, st));
	HIP_CHECK(hipMemcpyAsync(c0, c->d_ctr, sizeof c0, hipMemcpyDeviceToHost, st));
	nabwa_launch_dcache_insert(b->n, b->d_seq, b->d_rseq, b->d_poff, b->d_len, b->d_md, b->d_mg, b->d_status, b->d_naln, b->d_maxent, b->d_aln, b->P.aln_cap, b->d_wide_idx,
							   b->d_aln2, b->aln_cap2, b->d_grown_tab, row_cap, b->cache_mask, c->d_slots, c->n_slots, c->d_arena, c->arena_bytes, c->d_ctr, st);
	HIP_CHECK(hipMemcpyAsync(c1, c->d_ctr, sizeof c1, hipMemcpyDeviceToHost, st));
	HIP_CHECK(hipEventRecord(e1, st));
	HIP_CHECK(hipStreamSynchronize(st));
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipEventElapsedTime(&b->cache_insert_ms, e0, e1));
	c->used = c1[DC_USED]; c->entries = c1[DC_ENTRIES];
	b->n_inserted = c1[DC_ENTRIES] - c0[DC_ENTRIES];
	b->n_not_inserted = (c1[DC_FULL] - c0[DC_FULL]) + (c1[DC_SKIPPED] - c0[DC_SKIPPED]);
	if (getenv("NABWA_TIMING")) fprintf(stderr, "[nabwa] dedup cache: %d reads searched, %llu entered, %llu not (cache full or over %d rows), stage %.3f ms; %llu entries, %llu bytes\n",
										b->n, (unsigned long long)b->n_inserted, (unsigned long long)b->n_not_inserted, row_cap, b->cache_insert_ms, c1[DC_ENTRIES], c1[DC_USED]);
	return NABWA_OK;
}

static int sync_searches(nabwa_batch_t *b, int *n_second_pass);

extern "C" int nabwa_batch_sync(nabwa_batch_t *b, int *n_second_pass)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null batch");
	HIP_CHECK(hipSetDevice(b->ix->device));
	if (n_second_pass) *n_second_pass = 0;
	if (b->n == 0) return NABWA_OK;
	if (int r = sync_searches(b, n_second_pass)) return r;
	return b->cache && b->ran && !b->cache_inserted ? cache_insert(b) : NABWA_OK;
}

static int sync_searches(nabwa_batch_t *b, int *n_second_pass)
{
	unsigned int novf = 0;
	HIP_CHECK(hipMemcpyAsync(&novf, b->d_novf, 4, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipStreamSynchronize(b->stream));
	if (int r = w_stats_collect(b)) return r;
	HIP_CHECK(hipEventElapsedTime(&b->last_ms, b->ev0, b->ev1));
	HIP_CHECK(hipEventElapsedTime(&b->last_ms_w, b->evw, b->ev0));
	if (n_second_pass) *n_second_pass = (int)novf;
	if (novf == 0) return NABWA_OK;
	const bool timing = getenv("NABWA_TIMING") != 0;
	unsigned int cur = novf;
	b->deep_ran = 0; b->last_ms_deep = 0.f;
	if (env_int("NABWA_TIER_A", 0) && b->P.cap < 65534 && b->deep_only == 0)
		if (int r = tier_a_rerun(b, &cur, timing)) return r;
	return cur ? deep_searches(b, cur, timing) : NABWA_OK;
}

extern "C" float nabwa_batch_last_kernel_ms(nabwa_batch_t *b) { return b ? b->last_ms : 0.f; }
extern "C" float nabwa_batch_last_width_ms(nabwa_batch_t *b) { return b ? b->last_ms_w : 0.f; }
extern "C" float nabwa_batch_last_deep_ms(nabwa_batch_t *b) { return b ? b->last_ms_deep : 0.f; }

/* One extra, untimed run of both passes with the instrumented kernel: total Occ-bucket touches the
 * REFERENCE algorithm performs on this batch (the "algorithmic bytes" of the roofline are 48 B each). */
extern "C" int nabwa_batch_count_touches(nabwa_batch_t *b, uint64_t *n_bucket, uint64_t *n_bucket_width)
{
	if (!b || !n_bucket) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(b->ix->device));
	HIP_CHECK(hipMemsetAsync(b->d_sum, 0, TS_WORDS * sizeof(unsigned long long), b->stream));
	b->P.touch_counter = b->d_sum;
	/* the reference walks every exact tail row by row: count with the tail jump off (NABWA_TRIP_STATS=jump keeps it
	 * on to profile the production trips; the touch totals are then not the reference's) */
	const uint32_t kt0 = b->P.bwt[0].kmer_T, kt1 = b->P.bwt[1].kmer_T; const int tm0 = b->P.text_mode;
	const char *ts = getenv("NABWA_TRIP_STATS");
	if (!(ts && strcmp(ts, "jump") == 0)) { b->P.bwt[0].kmer_T = b->P.bwt[1].kmer_T = 0; b->P.text_mode = 0; }
	int r = nabwa_batch_run(b);
	if (r == NABWA_OK) r = nabwa_batch_sync(b, 0);
	b->P.touch_counter = 0;
	b->P.bwt[0].kmer_T = kt0; b->P.bwt[1].kmer_T = kt1; b->P.text_mode = tm0;
	if (r != NABWA_OK) return r;
	unsigned long long t[TS_WORDS];
	HIP_CHECK(hipMemcpy(t, b->d_sum, sizeof t, hipMemcpyDeviceToHost));
	*n_bucket = t[TS_TOUCH_S];                          /* search kernel (bwt_match_gap) */
	if (n_bucket_width) *n_bucket_width = t[TS_TOUCH_W];  /* width kernel (bwt_cal_width) */
	if (getenv("NABWA_TRIP_STATS") && b->class_sort) {
		unsigned int c[NCLS_WORDS];
		HIP_CHECK(hipMemcpy(c, b->d_ncls, sizeof c, hipMemcpyDeviceToHost));
		fprintf(stderr, "[nabwa] read classes by restarts 0 / 1 / 2+: %u / %u / %u\n", c[NCLS_SIZE + 0], c[NCLS_SIZE + 1], c[NCLS_SIZE + 2]);
	}
	if (getenv("NABWA_TRIP_STATS")) {
		fprintf(stderr, "[nabwa] search kernel: wave-trips %llu; lane-trips: expand %llu exact %llu entry-load %llu spec %llu query %llu two-bucket %llu exited %llu tail-jump %llu text-expand %llu text-tail %llu; longest read %llu trips, %llu reads over 2000 trips, %llu over 500\n",
				t[TS_TRIPS], t[TS_EXPAND], t[TS_EXACT], t[TS_ENT_LOAD], t[TS_SPEC], t[TS_QUERY], t[TS_TWO], t[TS_EXITED], t[TS_JUMP], t[TS_TEXT_EXPAND], t[TS_TEXT_TAIL],
				t[TS_MAX_TRIPS], t[TS_OVER_2000], t[TS_OVER_500]);
		fprintf(stderr, "[nabwa] the %llu reads over 8000 trips: %llu trips = expansions key-form %llu, rows two-bucket %llu, rows one-bucket %llu, text %llu (of all: %llu with gaps); pops %llu, tail steps %llu, jumps %llu\n",
				t[TS_LONG_READS], t[TS_LONG_TRIPS], t[TS_LONG_KF], t[TS_LONG_ROW2], t[TS_LONG_ROW1], t[TS_LONG_TEXT], t[TS_LONG_GAP], t[TS_LONG_POP], t[TS_LONG_TAIL], t[TS_LONG_JUMP]);
	}
	return NABWA_OK;
}

/* Tests: the records kernel W writes for reads [first, first + n), unpacked: per read and strand the len + 1 interval widths
 * and lower bounds of the full pass (bwt_cal_width, bwtaln.c:52-76, 123-124) and the seed_len + 1 bounds of the seed pass
 * (:126-130; only for reads longer than the seed).  Runs kernel W alone on a fresh record.  Rows are max_len + 1 wide. */
extern "C" int nabwa_batch_width_records(nabwa_batch_t *b, int first, int n, uint32_t *w_out, uint8_t *bid_out, uint8_t *seed_bid_out)
{
	if (!b || first < 0 || n < 0 || first + n > b->n_given || (n && (!w_out || !bid_out))) return nabwa_fail(NABWA_EINVAL, "bad argument");
	if (n == 0) return NABWA_OK;
	HIP_CHECK(hipSetDevice(b->ix->device));
	if (b->n_served) {      /* kernel W never saw a read served from the read cache: no records to give */
		std::vector<int32_t> m((size_t)n);
		HIP_CHECK(hipMemcpyAsync(m.data(), b->d_map + first, (size_t)n * 4, hipMemcpyDeviceToHost, b->stream));
		HIP_CHECK(hipStreamSynchronize(b->stream));
		for (int32_t v : m) if (v < 0) return nabwa_fail(NABWA_EINVAL, "nabwa_batch_width_records: the range holds a read served from the read cache (NABWA_DEDUP_CACHE), which has no width records");
	}
	HIP_CHECK(hipMemsetAsync(b->d_counter, 0, WC_WORDS * sizeof(unsigned int), b->stream));
	SearchParams PW = b->P; PW.ids = 0; PW.rd_cls = 0; PW.touch_counter = 0;
	if (int r = w_stats_arm(b, PW)) return r;
	nabwa_launch_fm_width(&PW, b->n_blocks_w, b->stream);
	HIP_CHECK(hipGetLastError());
	/* first and n are the caller's read indices: with a map (NABWA_DEDUP) the records of all reads searched come down and are picked from */
	std::vector<int32_t> src(b->d_map ? (size_t)n : 0);
	const size_t rec0 = b->d_map ? 0 : (size_t)first, n_rec = b->d_map ? (size_t)b->n : (size_t)n;
	std::vector<uint8_t> rec(n_rec * b->P.wstride);
	if (b->d_map) HIP_CHECK(hipMemcpyAsync(src.data(), b->d_map + first, (size_t)n * 4, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipMemcpyAsync(rec.data(), b->d_wdata + rec0 * b->P.wstride, rec.size(), hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipStreamSynchronize(b->stream));
	if (int r = w_stats_collect(b)) return r;
	const int W = b->max_len + 1, SW = b->opt.seed_len + 1;
	for (int i = 0; i < n; ++i) {
		const uint8_t *r = rec.data() + (size_t)(b->d_map ? src[i] : i) * b->P.wstride;
		for (int x = 0; x < 2; ++x) {
			memcpy(w_out + ((size_t)i * 2 + x) * W, (const uint32_t*)r + x * b->P.WL, 4 * (size_t)W);
			memcpy(bid_out + ((size_t)i * 2 + x) * W, r + b->P.woff_bid + x * b->P.WLB, (size_t)W);
			if (seed_bid_out && b->max_len > b->opt.seed_len && SW <= (int)b->P.SLB) memcpy(seed_bid_out + ((size_t)i * 2 + x) * SW, r + b->P.woff_sbid + x * b->P.SLB, (size_t)SW);
		}
	}
	return NABWA_OK;
}

extern "C" int nabwa_batch_checksum(nabwa_batch_t *b, uint64_t *sum, int64_t *n_rows)
{
	if (!b) return nabwa_fail(NABWA_EINVAL, "null batch");
	HIP_CHECK(hipSetDevice(b->ix->device));
	unsigned long long h[CKS_WORDS] = { 0, 0 };
	HIP_CHECK(hipMemsetAsync(b->d_sum, 0, sizeof h, b->stream));
	nabwa_launch_checksum(b->n_given, b->d_map, b->d_cent, b->cache ? b->cache->d_arena : nullptr, b->d_naln, b->d_aln, b->P.aln_cap, b->d_status, b->d_wide_idx, b->d_aln2, b->aln_cap2, b->d_grown_tab,
						  b->d_sum + CKS_SUM, b->d_sum + CKS_ROWS, b->stream);
	HIP_CHECK(hipMemcpyAsync(h, b->d_sum, sizeof h, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipStreamSynchronize(b->stream));
	if (sum) *sum = h[CKS_SUM];
	if (n_rows) *n_rows = (int64_t)h[CKS_ROWS];
	return NABWA_OK;
}

extern "C" int nabwa_batch_config(nabwa_batch_t *b, nabwa_batch_config_t *out)
{
	if (!b || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	memset(out, 0, sizeof(*out));
	out->n = b->n_given; out->min_len = b->min_len; out->max_len = b->max_len;
	out->deep_only = b->deep_only; out->ns1 = (int32_t)b->NS1; out->ns_wide = (int32_t)b->NS_wide;
	out->w_sync = b->P.w_sync; out->trip_budget = (int32_t)b->P.trip_budget; out->trip_budget_hard = (int32_t)b->P.trip_budget_hard;
	out->n_sync = out->hard_budget = -1;
	for (int q = 0; q < NCLS_N; ++q) out->cls[q] = -1;
	if (b->ran && b->class_sort) {
		HIP_CHECK(hipSetDevice(b->ix->device));
		unsigned int c[NCLS_WORDS];
		HIP_CHECK(hipMemcpyAsync(c, b->d_ncls, sizeof c, hipMemcpyDeviceToHost, b->stream));
		HIP_CHECK(hipStreamSynchronize(b->stream));
		for (int q = 0; q < NCLS_N; ++q) out->cls[q] = (int32_t)c[NCLS_SIZE + q];
		out->n_sync = (int32_t)c[NCLS_FIRST0];
		/* the rule of fm_search_kernel: the hard budget when most reads occur exactly on neither strand */
		if (!b->deep_only) out->hard_budget = b->P.trip_budget_hard && 2u * c[NCLS_FIRST0] > (uint32_t)b->n ? 1 : 0;
	}
	out->coop_lanes = b->deep_coop;
	out->lds_rd = b->deep_cfg ? (int32_t)b->deep_lds_rd : -1;
	return NABWA_OK;
}

/* the first n_words slots of the sure0 block (S0S_*, search_slots.hpp); zeros when NABWA_SURE0_STATS was not set at batch_create */
static int sure0_read(nabwa_batch_t *b, uint64_t *out, int n_words)
{
	if (!b || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int q = 0; q < n_words; ++q) out[q] = 0;
	if (!b->d_s0stats) return NABWA_OK;
	HIP_CHECK(hipSetDevice(b->ix->device));
	unsigned long long v[S0S_WORDS];
	HIP_CHECK(hipMemcpyAsync(v, b->d_s0stats, (size_t)n_words * sizeof v[0], hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipStreamSynchronize(b->stream));
	for (int q = 0; q < n_words; ++q) out[q] = v[q];
	return NABWA_OK;
}

/* NABWA_DEDUP: reads given, reads searched, reads whose hash met an earlier read's that they differ from (searched themselves), the switch */
extern "C" int nabwa_batch_dedup_stats(nabwa_batch_t *b, uint64_t out[4])
{
	if (!b || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	out[0] = (uint64_t)b->n_given; out[1] = (uint64_t)b->n; out[2] = b->dedup_coll; out[3] = b->dedup_on ? 1 : 0;
	return NABWA_OK;
}

/* the same four, then NABWA_DEDUP_CACHE: distinct reads served from the read cache, reads entered into it, reads not entered (cache full, over
 * the row cap, or the cache emptied for other options meanwhile), 1 if the batch went without the cache because of its option block */
extern "C" int nabwa_batch_dedup_stats_ex(nabwa_batch_t *b, uint64_t out[8])
{
	if (int r = nabwa_batch_dedup_stats(b, out)) return r;
	out[4] = (uint64_t)b->n_served; out[5] = b->n_inserted; out[6] = b->n_not_inserted; out[7] = b->cache_bypass ? 1 : 0;
	return NABWA_OK;
}

extern "C" int nabwa_batch_sure0_stats(nabwa_batch_t *b, uint64_t out[4]) { return sure0_read(b, out, 4); }      /* the first entry of the ABI: four words, S0S_READS .. S0S_NET */
extern "C" int nabwa_batch_sure0_stats_ex(nabwa_batch_t *b, uint64_t out[8]) { return sure0_read(b, out, S0S_WORDS); }

extern "C" int nabwa_batch_fetch(nabwa_batch_t *b, int32_t *n_aln, nabwa_aln1_t *aln_out, int64_t aln_cap, int64_t *n_rows,
								 int32_t *max_entries)
{
	if (!b || !n_aln) return nabwa_fail(NABWA_EINVAL, "null argument");
	HIP_CHECK(hipSetDevice(b->ix->device));
	if (n_rows) *n_rows = 0;
	if (b->n_given == 0) return NABWA_OK;      /* (b->n == 0 alone: every read is served from the read cache, and has rows to fetch) */
	// device-side compaction: exclusive scan of n_aln, then gather rows
	PoolBuf<uint32_t> d_off; PoolBuf<void> d_tmp; size_t tmp_bytes = 0; PoolBuf<uint4> d_rows; PoolBuf<int32_t> d_cnt;
	StreamDrain drain{ b->stream };
	const int n = b->n_given;
	/* with a map (NABWA_DEDUP) the caller's reads take the counts, max_entries and rows of the reads searched for them */
	const int32_t *naln = b->d_naln, *maxent = b->d_maxent;
	if (b->d_map) {
		HIP_CHECK(d_cnt.get(b->ix, (size_t)n * 8));
		nabwa_launch_dedup_expand(n, b->d_map, b->d_naln, b->d_maxent, b->d_cent, b->cache ? b->cache->d_arena : nullptr, d_cnt, d_cnt + n, b->stream);
		naln = d_cnt; maxent = d_cnt + n;
	}
	HIP_CHECK(d_off.get(b->ix, (size_t)(n + 1) * 4));
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp_bytes, (const uint32_t*)naln, d_off.p, n, b->stream));
	HIP_CHECK(d_tmp.get(b->ix, tmp_bytes ? tmp_bytes : 16));
	HIP_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp.p, tmp_bytes, (const uint32_t*)naln, d_off.p, n, b->stream));
	uint32_t last_off = 0; int32_t last_n = 0;
	HIP_CHECK(hipMemcpyAsync(&last_off, d_off + (n - 1), 4, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipMemcpyAsync(&last_n, naln + (n - 1), 4, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipMemcpyAsync(n_aln, naln, (size_t)n * 4, hipMemcpyDeviceToHost, b->stream));
	if (max_entries) HIP_CHECK(hipMemcpyAsync(max_entries, maxent, (size_t)n * 4, hipMemcpyDeviceToHost, b->stream));
	HIP_CHECK(hipStreamSynchronize(b->stream));
	const int64_t total = (int64_t)last_off + last_n;
	if (n_rows) *n_rows = total;
	int rc = NABWA_OK;
	if (total > aln_cap || (total && !aln_out)) rc = nabwa_fail(NABWA_ECAP, "aln_cap too small");
	else if (total) {
		HIP_CHECK(d_rows.get(b->ix, (size_t)total * 16));
		nabwa_launch_gather(n, b->d_map, b->d_cent, b->cache ? b->cache->d_arena : nullptr, b->d_naln, d_off, b->d_aln, b->P.aln_cap, b->d_status, b->d_wide_idx, b->d_aln2, b->aln_cap2, b->d_grown_tab,
							d_rows, b->stream);
		HIP_CHECK(hipMemcpyAsync(aln_out, d_rows, (size_t)total * 16, hipMemcpyDeviceToHost, b->stream));
		HIP_CHECK(hipStreamSynchronize(b->stream));
		HIP_CHECK(d_rows.release());
	}
	HIP_CHECK(d_off.release()); HIP_CHECK(d_tmp.release()); HIP_CHECK(d_cnt.release());
	return rc;
}
