// nabwa_index.hip -- the FM-index on the device: construction from the reference's arrays, loading, read-back, and the small
// per-row entries (bwt_sa, bwt_occ4).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <memory>
#include <string>
#include <vector>
#include "../../include/nabwa.h"
#include "launchers.hpp"
#include "dedup_cache_body.hpp"
#include "nabwa_internal.hpp"
#include "dev_pool.hpp"
#include "finish_gpu.hpp"

static int build_one(nabwa_index *ix, int t_, const uint32_t *words, uint64_t n_words, bool on_device,
					 const uint32_t *sa_words, uint64_t n_sa_words)
{
	uint32_t hdr[5];
	if (n_words < 5) return nabwa_fail(NABWA_EIO, "bwt array too short");
	if (on_device) HIP_CHECK(hipMemcpy(hdr, words, 20, hipMemcpyDeviceToHost)); else memcpy(hdr, words, 20);
	DevBwt &B = ix->bwt[t_];
	memset(&B, 0, sizeof(B));
	memset(ix->kmer_pk[t_], 0xff, sizeof ix->kmer_pk[t_]);
	B.primary = hdr[0]; B.L2[0] = 0; B.L2[1] = hdr[1]; B.L2[2] = hdr[2]; B.L2[3] = hdr[3]; B.seq_len = hdr[4];
	/* the reference's loader computes n_sa = (seq_len + sa_intv) / sa_intv in 32 bits (bwtio.c:175, bwt.c:56): above this it wraps */
	if (B.seq_len > 0xffffffdfu) return nabwa_fail(NABWA_EINVAL, "seq_len above 0xffffffdf: the reference's SA count wraps (bwtio.c:175)");
	/* (seq_len+15)/16 BWT words plus (seq_len+127)/128+1 checkpoints of 4 words (bwtmisc.c:130-131) */
	const uint64_t expect = ((uint64_t)B.seq_len + 15) / 16 + (((uint64_t)B.seq_len + 127) / 128 + 1) * 4;
	if (n_words - 5 < expect) return nabwa_fail(NABWA_EIO, "bwt array shorter than its seq_len implies");
	B.n_buckets = (uint32_t)(((uint64_t)B.seq_len + NABWA_INTV - 1) / NABWA_INTV);
	DevBuf raw;
	const uint32_t *src = words + 5;
	if (!on_device) {
		if (int r = raw.get((n_words - 5) * 4)) return r;
		HIP_CHECK(hipMemcpy(raw.p, words + 5, (n_words - 5) * 4, hipMemcpyHostToDevice));
		src = raw.as<uint32_t>();
	}
	HIP_CHECK(hipMalloc(&ix->bk[t_], (size_t)B.n_buckets * 64));
	nabwa_launch_repack(src, B.seq_len, B.n_buckets, ix->bk[t_], 0);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipDeviceSynchronize());
	HIP_CHECK(raw.release());
	B.bk = ix->bk[t_];
	ix->bytes += (uint64_t)B.n_buckets * 64;
	{	/* interval table, ALL levels 1..T back to back (level t at offset (4^t - 4) / 3): T = floor(log4(seq_len)) + 1 (about a
		 * quarter row per key at the last level: most walks that the table replaces die inside it), at most 16 and no more
		 * than 40 % of the free HBM; NABWA_KMER_T overrides (0 = off).  GRCh38: T = 16, 46 GB per index.  The search keeps
		 * every gap-free entry of depth <= T as its path KEY and takes children, tails and forced walks from here. */
		int T = 0;
		for (uint64_t x = B.seq_len; x >= 4; x >>= 2) ++T;
		T += 1;
		const char *e = getenv("NABWA_KMER_T");
		if (e) T = atoi(e);
		if (T > 16) T = 16;
		size_t free_b = 0, total_b = 0;
		HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
		auto table_entries = [](int t) { size_t x = 0; for (int u = 1; u <= t; ++u) x += (size_t)1 << (2 * u); return x; };
		/* both directions must get the same depth (the search runs without tables otherwise): the first one built decides, leaving
		 * room for the second; the second takes that depth, and says so loudly if it cannot */
		if (ix->kmer_T_pick < 0) {
			while (T > 12 && 2 * table_entries(T) * 8 > free_b / 5 * 3) --T;
			ix->kmer_T_pick = T;
		} else {
			T = ix->kmer_T_pick;
			if (T >= 1 && table_entries(T) * 8 > free_b / 10 * 9) {
				fprintf(stderr, "[nabwa] WARNING: no device memory for the second interval table of depth %d (%zu MB free): the search runs WITHOUT interval tables "
								"(several times slower); free device memory or set NABWA_KMER_T lower\n", T, free_b >> 20);
				T = 0;
			}
		}
		if (T >= 1) {
			const size_t lo_n = table_entries(T);
			HIP_CHECK(hipMalloc(&ix->kmer[t_], lo_n * 8));
			uint2 *prev = 0, *cur = ix->kmer[t_];
			for (int t = 1; t <= T; ++t) {
				nabwa_launch_kmer_level(&B, prev, cur, (uint64_t)1 << (2 * t), 0);
				prev = cur; cur += (size_t)1 << (2 * t);
			}
			/* the primary key of every level, for kernel W's widths by summing (fm_index.hip: kmer_primary_kernel) */
			DevBuf pk;
			if (int r = pk.get(sizeof ix->kmer_pk[t_])) return r;
			HIP_CHECK(hipMemsetAsync(pk.p, 0xff, sizeof ix->kmer_pk[t_], 0));
			for (int t = 1; t <= T; ++t)
				nabwa_launch_kmer_primary(ix->kmer[t_] + table_entries(t - 1), (uint64_t)1 << (2 * t), B.primary, pk.as<uint32_t>() + t, 0);
			HIP_CHECK(hipGetLastError());
			HIP_CHECK(hipMemcpy(ix->kmer_pk[t_], pk.p, sizeof ix->kmer_pk[t_], hipMemcpyDeviceToHost));
			HIP_CHECK(hipDeviceSynchronize());
			HIP_CHECK(pk.release());
			ix->bytes += lo_n * 8;
			B.kmer = prev; B.kmer_T = (uint32_t)T; B.kmer_lo = ix->kmer[t_]; B.kmer_LW = (uint32_t)T;
		}
	}
	if (sa_words) {
		uint32_t sh[7];
		if (n_sa_words < 7) return nabwa_fail(NABWA_EIO, "sa array too short");
		if (on_device) HIP_CHECK(hipMemcpy(sh, sa_words, 28, hipMemcpyDeviceToHost)); else memcpy(sh, sa_words, 28);
		if (sh[0] != B.primary || sh[6] != B.seq_len) return nabwa_fail(NABWA_EIO, "SA-BWT inconsistency");   /* bwtio.c:169,173 */
		B.sa_intv = sh[5];
		/* n_sa = (seq_len + sa_intv) / sa_intv is 32-bit in the reference's loader (bwtio.c:175): 0xffffffdf above holds for its interval of
		 * 32, a larger interval wraps sooner */
		if (B.sa_intv < 1 || (uint64_t)B.seq_len + B.sa_intv > 0xffffffffull)
			return nabwa_fail(NABWA_EINVAL, "seq_len + sa_intv above 0xffffffff: the reference's SA count wraps (bwtio.c:175)");
		B.n_sa = (uint32_t)(((uint64_t)B.seq_len + B.sa_intv) / B.sa_intv);
		if (n_sa_words - 7 < (uint64_t)B.n_sa - 1) return nabwa_fail(NABWA_EIO, "sa array shorter than n_sa");
		HIP_CHECK(hipMalloc(&ix->sa[t_], (size_t)B.n_sa * 4));
		HIP_CHECK(hipMemset(ix->sa[t_], 0xff, 4));
		HIP_CHECK(hipMemcpy(ix->sa[t_] + 1, sa_words + 7, (size_t)(B.n_sa - 1) * 4,
						 on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice));
		B.sa = ix->sa[t_];
		ix->bytes += (uint64_t)B.n_sa * 4;
		const char *tm = getenv("NABWA_TEXT_MODE");
		if (!(tm && atoi(tm) == 0)) {      /* full SA + inverse + text, ~8.3 B per base (NABWA_TEXT_MODE=0: keep the samples only) */
			const size_t rows = (size_t)B.seq_len + 1, words = ((size_t)B.seq_len + 15) / 16 + 4;
			DevBuf tb;
			HIP_CHECK(hipMalloc(&ix->sa_full[t_], rows * 4)); HIP_CHECK(hipMalloc(&ix->isa[t_], rows * 4));
			HIP_CHECK(hipMalloc(&ix->text[t_], words * 4)); if (int r = tb.get(rows)) return r;
			nabwa_launch_sa_fill(&B, ix->sa_full[t_], ix->isa[t_], tb.as<uint8_t>(), 0);
			nabwa_launch_text_pack(tb.as<uint8_t>(), B.seq_len, (uint32_t)words, ix->text[t_], 0);
			HIP_CHECK(hipGetLastError());
			HIP_CHECK(hipDeviceSynchronize());
			HIP_CHECK(tb.release());
			B.sa_full = ix->sa_full[t_]; B.isa = ix->isa[t_]; B.text = ix->text[t_];
			ix->bytes += rows * 8 + words * 4;
		}
	}
	return NABWA_OK;
}

extern "C" int nabwa_index_from_arrays(int device, int is_device, const uint32_t *bwt0, uint64_t nw0,
									   const uint32_t *bwt1, uint64_t nw1, const uint32_t *sa0, uint64_t ns0,
									   const uint32_t *sa1, uint64_t ns1, nabwa_index_t **out)
{
	if (!out || !bwt0 || !bwt1) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (nabwa_device_count() <= device) return nabwa_fail(NABWA_ENODEV, "no such HIP device");
	HIP_CHECK(hipSetDevice(device));
	nabwa_index *ix = new nabwa_index();
	ix->pool = pool_create();
	ix->device = device;
	int r = build_one(ix, 0, bwt0, nw0, is_device != 0, sa0, ns0);
	if (r == NABWA_OK) r = build_one(ix, 1, bwt1, nw1, is_device != 0, sa1, ns1);
	if (r != NABWA_OK) { nabwa_index_destroy(ix); return r; }
	*out = ix;
	return NABWA_OK;
}

static bool slurp(const std::string &fn, std::vector<uint32_t> &v)
{
	FILE *f = fopen(fn.c_str(), "rb");
	if (!f) return false;
	fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
	v.resize((n + 3) / 4);
	bool ok = fread(v.data(), 1, n, f) == (size_t)n;
	fclose(f);
	return ok;
}

extern "C" int nabwa_index_load(const char *prefix, int device, int with_sa, int with_pac, nabwa_index_t **out)
{
	if (!prefix || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	std::vector<uint32_t> b0, b1, s0, s1;
	std::string p(prefix);
	if (!slurp(p + ".bwt", b0)) return nabwa_fail(NABWA_EIO, "cannot read %s.bwt", prefix);
	if (!slurp(p + ".rbwt", b1)) return nabwa_fail(NABWA_EIO, "cannot read %s.rbwt", prefix);
	if (with_sa) {
		if (!slurp(p + ".sa", s0)) return nabwa_fail(NABWA_EIO, "cannot read %s.sa", prefix);
		if (!slurp(p + ".rsa", s1)) return nabwa_fail(NABWA_EIO, "cannot read %s.rsa", prefix);
	}
	int r = nabwa_index_from_arrays(device, 0, b0.data(), b0.size(), b1.data(), b1.size(),
									with_sa ? s0.data() : 0, s0.size(), with_sa ? s1.data() : 0, s1.size(), out);
	if (r == NABWA_OK && with_pac) {
		r = nabwa_index_attach_reference(*out, prefix);
		if (r != NABWA_OK) { nabwa_index_destroy(*out); *out = 0; }
	}
	return r;
}

extern "C" void nabwa_index_destroy(nabwa_index_t *ix)
{
	if (!ix) return;
	(void)hipSetDevice(ix->device);
	for (int t = 0; t < 2; ++t) { if (ix->bk[t]) (void)hipFree(ix->bk[t]); if (ix->sa[t]) (void)hipFree(ix->sa[t]); if (ix->kmer[t]) (void)hipFree(ix->kmer[t]); if (ix->kmer_top[t]) (void)hipFree(ix->kmer_top[t]);
		if (ix->sa_full[t]) (void)hipFree(ix->sa_full[t]); if (ix->isa[t]) (void)hipFree(ix->isa[t]); if (ix->text[t]) (void)hipFree(ix->text[t]); }
	nabwa_finish_drop_reference(ix);
	if (nabwa_dedup_cache *c = ix->dcache) {      /* (pool buffers: back to the pool, which goes next) */
		if (c->d_slots) (void)pool_free(ix, c->d_slots);
		if (c->d_arena) (void)pool_free(ix, c->d_arena);
		if (c->d_ctr) (void)pool_free(ix, c->d_ctr);
		delete c;
	}
	pool_destroy(ix->pool);
	if (ix->d_ntpac) (void)hipFree(ix->d_ntpac);
	delete ix->ref_nt;
	delete ix->ref;
	delete ix;
}

/* Read-back of the derived index parts (tests): what 0 = sa_full[first..), 1 = isa[first..), 2 = text bases first.. (one per
 * word), 3 = interval table, level kmer_T: entry pairs {k, l} of keys first.. (2 words each), 4 = kmer_T (one word), 5 = the primary keys of
 * levels first.. (level 0..16; ~0u: none). */
extern "C" int nabwa_index_export(const nabwa_index_t *ix, int which, int what, uint64_t first, uint64_t n, uint32_t *out)
{
	if (!ix || !out || which < 0 || which > 1) return nabwa_fail(NABWA_EINVAL, "bad argument");
	HIP_CHECK(hipSetDevice(ix->device));
	const DevBwt &B = ix->bwt[which];
	if (what == 4) { out[0] = B.kmer_T; return NABWA_OK; }
	if (what == 5) {
		if (first + n > NABWA_PK_LEVELS) return nabwa_fail(NABWA_EINVAL, "out of range");
		memcpy(out, ix->kmer_pk[which] + first, n * 4);
		return NABWA_OK;
	}
	if (what == 3) {
		if (!B.kmer || first + n > (1ull << (2 * B.kmer_T))) return nabwa_fail(NABWA_EINVAL, "no interval table / out of range");
		HIP_CHECK(hipMemcpy(out, B.kmer + first, n * 8, hipMemcpyDeviceToHost));
		return NABWA_OK;
	}
	if (!B.sa_full) return nabwa_fail(NABWA_EINVAL, "index has no text-mode companions (no SA given, or NABWA_TEXT_MODE=0)");
	if (what == 0 || what == 1) {
		if (first + n > (uint64_t)B.seq_len + 1) return nabwa_fail(NABWA_EINVAL, "out of range");
		HIP_CHECK(hipMemcpy(out, (what ? B.isa : B.sa_full) + first, n * 4, hipMemcpyDeviceToHost));
		return NABWA_OK;
	}
	if (what == 2) {
		if (first + n > (uint64_t)B.seq_len) return nabwa_fail(NABWA_EINVAL, "out of range");
		const uint64_t w0 = first / 16, w1 = (first + n + 15) / 16;
		std::vector<uint32_t> w(w1 - w0);
		HIP_CHECK(hipMemcpy(w.data(), B.text + w0, (w1 - w0) * 4, hipMemcpyDeviceToHost));
		for (uint64_t j = 0; j < n; ++j) { const uint64_t p = first + j; out[j] = w[p / 16 - w0] >> (2 * (p & 15)) & 3u; }
		return NABWA_OK;
	}
	return nabwa_fail(NABWA_EINVAL, "unknown part");
}

extern "C" uint32_t nabwa_index_seq_len(const nabwa_index_t *ix, int which) { return ix->bwt[which & 1].seq_len; }
extern "C" uint64_t nabwa_index_device_bytes(const nabwa_index_t *ix) { return ix->bytes; }

/* ------------------------------------------------------------------ the read cache of NABWA_DEDUP_CACHE */

/* A budget of B bytes: the table takes the largest power of two of slots within B / 8 bytes (at least 1024 slots), the arena the rest.  An entry
 * of a 100 bp read with one row is 272 bytes, of a 30 bp read 112: with entries of 128 bytes and more the table is at most half full when
 * the arena is. */
int nabwa_dcache_get(nabwa_index *ix, long mib, nabwa_dedup_cache **out)
{
	std::lock_guard<std::mutex> lk(ix->dcache_mu);
	if (ix->dcache) { *out = ix->dcache; return NABWA_OK; }
	uint64_t budget = (uint64_t)mib << 20;
	size_t free_b = 0, total_b = 0;
	HIP_CHECK(hipMemGetInfo(&free_b, &total_b));
	{ std::lock_guard<std::mutex> pk(ix->pool->mu); free_b += ix->pool->idle_bytes; }      /* (the pool gives its idle buffers back when an allocation fails) */
	if (budget > free_b) {
		char why[160]; snprintf(why, sizeof why, "NABWA_DEDUP_CACHE=%ld: more MiB than the device has free (%zu)", mib, free_b >> 20);
		return nabwa_fail(NABWA_EINVAL, "%s", why);
	}
	if (budget > (65535ull << 20)) budget = 65535ull << 20;      /* a batch names an entry by its arena offset / 16 in 32 bits */
	uint32_t n_slots = 1024;
	while ((uint64_t)n_slots * 2 * 8 <= budget / 8 && n_slots < (1u << 30)) n_slots *= 2;
	const uint64_t ctr_bytes = DC_WORDS * sizeof(unsigned long long);
	const uint64_t arena_bytes = (budget - (uint64_t)n_slots * 8 - ctr_bytes) & ~(uint64_t)15;
	std::unique_ptr<nabwa_dedup_cache> c(new nabwa_dedup_cache());
	hipError_t e = pool_malloc(ix, (void**)&c->d_slots, (size_t)n_slots * 8);
	if (e == hipSuccess) e = pool_malloc(ix, (void**)&c->d_arena, arena_bytes);
	if (e == hipSuccess) e = pool_malloc(ix, (void**)&c->d_ctr, ctr_bytes);
	if (e == hipSuccess) e = hipMemset(c->d_slots, 0, (size_t)n_slots * 8);
	if (e == hipSuccess) e = hipMemset(c->d_ctr, 0, ctr_bytes);
	if (e != hipSuccess) {
		if (c->d_slots) (void)pool_free(ix, c->d_slots);
		if (c->d_arena) (void)pool_free(ix, c->d_arena);
		if (c->d_ctr) (void)pool_free(ix, c->d_ctr);
		return nabwa_hip_fail(e, "the device memory of NABWA_DEDUP_CACHE", __FILE__, __LINE__);
	}
	c->n_slots = n_slots; c->arena_bytes = arena_bytes; c->reserved = (uint64_t)n_slots * 8 + arena_bytes + ctr_bytes;
	ix->bytes += c->reserved;
	*out = ix->dcache = c.release();
	return NABWA_OK;
}

int nabwa_dcache_reset(nabwa_index *ix, nabwa_dedup_cache *c)
{
	(void)ix;
	HIP_CHECK(hipMemset(c->d_slots, 0, (size_t)c->n_slots * 8));      /* (the null stream: every lookup and insert stage has drained its own) */
	HIP_CHECK(hipMemset(c->d_ctr, 0, DC_WORDS * sizeof(unsigned long long)));
	HIP_CHECK(hipStreamSynchronize(0));
	c->has_sig = false; c->used = c->entries = 0;
	return NABWA_OK;
}

extern "C" int nabwa_index_dedup_cache_stats(nabwa_index_t *ix, uint64_t out[8])
{
	if (!ix || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (int q = 0; q < 8; ++q) out[q] = 0;
	nabwa_dedup_cache *c;
	{ std::lock_guard<std::mutex> lk(ix->dcache_mu); c = ix->dcache; }
	if (!c) return NABWA_OK;
	std::lock_guard<std::mutex> lk(c->mu);
	out[0] = c->reserved; out[1] = c->used; out[2] = c->entries; out[3] = c->n_slots;
	out[4] = c->lookups; out[5] = c->served; out[6] = c->flushes; out[7] = c->bypasses;
	return NABWA_OK;
}

extern "C" int nabwa_index_dedup_cache_clear(nabwa_index_t *ix)
{
	if (!ix) return nabwa_fail(NABWA_EINVAL, "null argument");
	nabwa_dedup_cache *c;
	{ std::lock_guard<std::mutex> lk(ix->dcache_mu); c = ix->dcache; }
	if (!c) return NABWA_OK;
	HIP_CHECK(hipSetDevice(ix->device));
	std::lock_guard<std::mutex> lk(c->mu);
	if (c->pins) return nabwa_fail(NABWA_EINVAL, "nabwa_index_dedup_cache_clear: live batches hold reads served from the cache");
	return nabwa_dcache_reset(ix, c);
}

/* ------------------------------------------------------------------ bwt_sa / occ batches */

extern "C" int nabwa_sa_lookup(nabwa_index_t *ix, int n, const uint8_t *which, const uint32_t *k, uint32_t *sa_out)
{
	if (!ix || n < 0 || (n && (!which || !k || !sa_out))) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (!ix->bwt[0].sa || !ix->bwt[1].sa) return nabwa_fail(NABWA_EINVAL, "index was loaded without suffix arrays");
	if (n == 0) return NABWA_OK;
	HIP_CHECK(hipSetDevice(ix->device));
	/* (buffers from the pool kept with the index: this is called once per batch by the finishing chains) */
	PoolBuf<uint8_t> dw; PoolBuf<uint32_t> dk, dout;
	StreamDrain drain{ 0 };
	HIP_CHECK(dw.get(ix, (size_t)n)); HIP_CHECK(dk.get(ix, (size_t)n * 4)); HIP_CHECK(dout.get(ix, (size_t)n * 4));
	HIP_CHECK(hipMemcpy(dw, which, n, hipMemcpyHostToDevice));
	HIP_CHECK(hipMemcpy(dk, k, (size_t)n * 4, hipMemcpyHostToDevice));
	nabwa_launch_sa_lookup(ix->bwt, n, dw, dk, dout, 0);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipMemcpy(sa_out, dout, (size_t)n * 4, hipMemcpyDeviceToHost));
	HIP_CHECK(dw.release()); HIP_CHECK(dk.release()); HIP_CHECK(dout.release());
	return NABWA_OK;
}

extern "C" int nabwa_occ4(nabwa_index_t *ix, int which, int n, const uint32_t *k, uint32_t *cnt_out)
{
	if (!ix || n < 0 || (n && (!k || !cnt_out))) return nabwa_fail(NABWA_EINVAL, "null argument");
	if (n == 0) return NABWA_OK;
	HIP_CHECK(hipSetDevice(ix->device));
	DevBuf dk, dout;
	if (int r = dk.get((size_t)n * 4)) return r;
	if (int r = dout.get((size_t)n * 16)) return r;
	HIP_CHECK(hipMemcpy(dk.p, k, (size_t)n * 4, hipMemcpyHostToDevice));
	nabwa_launch_occ4(&ix->bwt[which & 1], n, dk.as<uint32_t>(), dout.as<uint32_t>(), 0);
	HIP_CHECK(hipGetLastError());
	HIP_CHECK(hipMemcpy(cnt_out, dout.p, (size_t)n * 16, hipMemcpyDeviceToHost));
	HIP_CHECK(dk.release()); HIP_CHECK(dout.release());
	return NABWA_OK;
}
