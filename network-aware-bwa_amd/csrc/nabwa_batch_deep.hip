// nabwa_batch_deep.hip -- the host side of kernel D (fm_deep_body.hpp): one search per wavefront, arenas paged out of one pool.
// nabwa_batch_sync hands it the reads kernel S flagged.  (Round 1 re-ran them from scratch on one lane each in tiers of growing
// per-lane arenas: 22 k reads/s on the ancient-DNA workload, the launch as long as its longest search.)
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/nabwa.h"
#include "nabwa_batch.hpp"
#include "host_util.hpp"

// rows of the wide result arrays for the `cur` reads that are left
static int grow_wide_rows(nabwa_batch *b, unsigned int cur)
{
	if (b->n2 >= (int)cur && b->aln_cap2 == env_int("NABWA_ALNCAP2", 1024)) return NABWA_OK;
	(void)b->d_naln2.release(); (void)b->d_maxent2.release(); (void)b->d_status2.release(); (void)b->d_aln2.release();
	b->n2 = 0;
	b->aln_cap2 = env_int("NABWA_ALNCAP2", 1024);
	if (b->aln_cap2 < 1) b->aln_cap2 = 1;
	HIP_CHECK(b->d_naln2.get(b->ix, (size_t)cur * 4)); HIP_CHECK(b->d_maxent2.get(b->ix, (size_t)cur * 4));
	HIP_CHECK(b->d_status2.get(b->ix, cur)); HIP_CHECK(b->d_aln2.get(b->ix, (size_t)cur * b->aln_cap2 * 16));
	b->n2 = (int)cur;
	return NABWA_OK;
}

// kernel D's launch shape and pool size: worked out once per batch (device queries cost as much as a small launch)
static int deep_configure(nabwa_batch *b)
{
	const uint32_t NS = b->NS_wide;
	hipDeviceProp_t prop;
	HIP_CHECK(hipGetDeviceProperties(&prop, b->ix->device));
	uint32_t K = (uint32_t)env_int("NABWA_DEEP_STAGE", (int)DEEP_STAGE_MAX);
	if (K < 1u) K = 1u;
	if (K > DEEP_STAGE_MAX) K = DEEP_STAGE_MAX;
	// the read's own data (bound bytes, seed bound bytes, both strands' bases) sits in the wave's LDS when it is small enough
	const uint32_t rd_pl = align_up((uint32_t)(b->max_len > 0 ? b->max_len : 1), 16);
	uint32_t lds_rd = 2u * b->P.WLB + 2u * b->P.SLB + 2u * rd_pl;
	if (lds_rd > (uint32_t)env_int("NABWA_DEEP_LDS_MAX", 6144)) lds_rd = 0;
	int occ = nabwa_deep_occupancy((int)NS, (int)lds_rd);
	if (occ < 1) occ = 1;
	if (env_int("NABWA_DEEP_WAVES_PER_CU", 0) > 0) occ = env_int("NABWA_DEEP_WAVES_PER_CU", 0);
	size_t budget = (size_t)env_int("NABWA_DEEP_GB", 32) << 30;
	{
		size_t fr = 0, tot = 0;
		HIP_CHECK(hipMemGetInfo(&fr, &tot));
		size_t avail = fr;
		{ std::lock_guard<std::mutex> lk(b->ix->pool->mu); avail += b->ix->pool->idle_bytes; }
		avail = avail > ((size_t)6 << 30) ? avail - ((size_t)6 << 30) : ((size_t)64 << 20);
		if (budget > avail) budget = avail;
	}
	if (getenv("NABWA_DEEP_PAGES")) budget = (size_t)env_int("NABWA_DEEP_PAGES", 64) * ((size_t)DEEP_PAGE * 16 + 4);     /* (tests: a pool that runs dry) */
	size_t n_pages = budget / ((size_t)DEEP_PAGE * 16 + 4);
	if (n_pages > 0xfffffff0ull) n_pages = 0xfffffff0ull;
	if (n_pages < 2) n_pages = 2;
	// pages one search can hold at most: its live entries are bounded by the cut-off (bwtgap.c:140) plus one round's
	// children, and every score level may have a partly filled page
	uint64_t cap_pages = ((uint64_t)(b->opt.max_entries > 0 ? b->opt.max_entries : 0) + 9ull * 64ull * K + 2) / DEEP_PAGE + NS + 4;
	if (cap_pages > n_pages) cap_pages = n_pages;
	b->deep_K = K; b->deep_lds_rd = lds_rd; b->deep_rd_pl = rd_pl; b->deep_n_pages = n_pages; b->deep_cap_pages = cap_pages;
	b->deep_waves_max = (long)prop.multiProcessorCount * occ;
	b->deep_cfg = 1;
	return NABWA_OK;
}

// kernel D's page pool, per-wave page lists and staging, and its counters, at the configured sizes for n_waves waves
static int deep_grow_buffers(nabwa_batch *b, long n_waves)
{
	const size_t n_pages = b->deep_n_pages;
	if (b->deep_pages < n_pages) {
		b->deep_pages = 0;
		HIP_CHECK(b->d_pages.release()); HIP_CHECK(b->d_page_prev.release());
		HIP_CHECK(b->d_pages.get(b->ix, n_pages * DEEP_PAGE * 16)); HIP_CHECK(b->d_page_prev.get(b->ix, n_pages * 4));
		b->deep_pages = n_pages;
	}
	const size_t own_words = (size_t)n_waves * 2 * b->deep_cap_pages, stage_ent = (size_t)n_waves * 64 * b->deep_K * 4;
	if (b->deep_own_words < own_words) {
		b->deep_own_words = 0;
		HIP_CHECK(b->d_deep_own.release());
		HIP_CHECK(b->d_deep_own.get(b->ix, own_words * 4)); b->deep_own_words = own_words;
	}
	if (b->deep_stage_ent < stage_ent) {
		b->deep_stage_ent = 0;
		HIP_CHECK(b->d_deep_stage.release());
		HIP_CHECK(b->d_deep_stage.get(b->ix, stage_ent * 16)); b->deep_stage_ent = stage_ent;
	}
	if (!b->d_deep_ctr) HIP_CHECK(b->d_deep_ctr.get(b->ix, DS_WORDS * sizeof(unsigned long long)));
	return NABWA_OK;
}

// kernel D's parameters for the reads in d_ovf_ids, results into the wide rows (and, for nabwa_batch_config, the coop setting they came to)
static void deep_fill_params(nabwa_batch *b, DeepParams &D, bool stats)
{
	memset(&D, 0, sizeof(D));
	D.S = b->P;
	D.S.ids = b->d_ovf_ids; D.S.n_sync = 0; D.S.w_sync = 0; D.S.res_slot = b->d_wide_idx;
	D.S.n_aln = b->d_naln2; D.S.max_ent = b->d_maxent2; D.S.status = b->d_status2; D.S.aln = b->d_aln2; D.S.aln_cap = b->aln_cap2;
	D.pages = b->d_pages; D.page_prev = b->d_page_prev; D.n_pages = (uint32_t)b->deep_n_pages;
	D.page_bump = (unsigned int*)(b->d_deep_ctr + DS_PAGE_BUMP);
	D.own = b->d_deep_own; D.own_cap = (uint32_t)b->deep_cap_pages; D.stage = b->d_deep_stage; D.stage_k = b->deep_K;
	D.NS = b->NS_wide; D.lds_rd = b->deep_lds_rd; D.rd_pl = b->deep_rd_pl;
	D.careful_all = env_int("NABWA_DEEP_CAREFUL", 0); D.max_lanes = env_int("NABWA_DEEP_LANES", 64);
	/* key-form entries (fm_deep.hpp): both indexes carry interval tables of one depth, and no row number reaches the form's marker;
	 * NABWA_DEEP_KEYFORM=0 keeps every entry as rows (A/B runs, and what the touch-counting run does anyway) */
	{
		const DevBwt &B0 = b->P.bwt[0], &B1 = b->P.bwt[1];
		const bool ok = B0.kmer_T > 0 && B0.kmer_T == B1.kmer_T && B0.kmer_LW == B0.kmer_T && B1.kmer_LW == B1.kmer_T && B0.kmer_lo && B1.kmer_lo &&
						B0.seq_len < DEEP_KEYL - 1u && B1.seq_len < DEEP_KEYL - 1u && (b->P.text_mode & 4) && env_int("NABWA_DEEP_KEYFORM", 1);
		D.key_T = ok ? B0.kmer_T : 0u;
	}
	if (D.max_lanes < 1) D.max_lanes = 1;
	if (D.max_lanes > 64) D.max_lanes = 64;

	D.stats = stats ? b->d_deep_ctr.p : 0;
	D.hist = env_int("NABWA_DEEP_HIST", 0);
	/* the wave-wide expansion of one-row chains pays where chains are long: reads of 100 bases and more (PE D -24 %); on reads of 50-76 bases
	 * its chains end after a level or two, and the kernel built without it is the faster one (profiles/r03_deep_variants.txt) */
	D.coop_lanes = (uint32_t)env_int("NABWA_DEEP_COOP", b->max_len >= 90 ? 4 : 0);
	b->deep_coop = (int)D.coop_lanes;
}

/* One launch of kernel D over the first n_reads reads of d_ovf_ids on `waves` waves: their width records again, both counter blocks
 * cleared, the launch, its results scattered into the per-read arrays -- from the wide rows (D.S.res_slot set), or from a grown
 * block that D.S.aln names (res_slot null) -- and the reads it could not finish collected: *left of them, status NABWA_ST_POOL
 * after a search on the wide rows, NABWA_ST_HITCAP after one on a grown block.  first: the first pass over these reads (kernel S
 * had them before: clean records are skipped; the launch is the one timed). */
static int deep_launch(nabwa_batch *b, DeepParams &D, unsigned int n_reads, long waves, bool first, unsigned int *left)
{
	const bool grown = !D.S.res_slot;
	D.S.n = (int)n_reads;
	rebuild_widths(b, D.S, n_reads, first);
	HIP_CHECK(hipMemsetAsync(b->d_counter, 0, WC_WORDS * sizeof(unsigned int), b->stream));
	HIP_CHECK(hipMemsetAsync(b->d_deep_ctr, 0, DS_WORDS * sizeof(unsigned long long), b->stream));
	D.S.work_counter = b->d_counter;
	if (first) HIP_CHECK(hipEventRecord(b->evd0, b->stream));
	nabwa_launch_fm_deep(&D, (int)waves, b->stream);
	if (first) HIP_CHECK(hipEventRecord(b->evd1, b->stream));
	if (grown) {
		nabwa_launch_scatter_grown((int)n_reads, b->d_ovf_ids, D.S.n_aln, D.S.max_ent, D.S.status, b->d_naln, b->d_maxent, b->d_status, b->d_wide_idx,
								   D.S.aln, (size_t)D.S.aln_cap, b->d_grown_tab, b->grown_used, b->stream);
		b->grown_used += (int)n_reads;
	} else
		nabwa_launch_scatter_wide((int)n_reads, b->d_ovf_ids, D.S.n_aln, D.S.max_ent, D.S.status, b->d_naln, b->d_maxent, b->d_status, b->d_wide_idx, b->stream);
	HIP_CHECK(hipGetLastError());
	return recollect(b, grown ? NABWA_ST_HITCAP : NABWA_ST_POOL, left);
}

/* kernel D's statistics of one launch (st: its DS_WORDS counters, search_slots.hpp), as NABWA_TIMING prints them */
static void deep_print_stats(const unsigned long long *st, int hist, bool guaranteed, unsigned int todo, long waves, size_t n_pages, unsigned int n_pool, double secs)
{
	fprintf(stderr, "[nabwa] kernel D%s: %u reads on %ld waves (%zu pages of 4 KB, %u handed out), %u left for the guaranteed pass, %.3f s; rounds %llu, chains run %llu / committed %llu, wave-steps %llu, careful rounds %llu, exact tails: %llu rank steps, %llu finished by text; longest read %.3f s / %llu rounds, all reads %.1f wave-s, longest wave %.3f s\n",
			guaranteed ? " (guaranteed pass)" : "", todo, waves, n_pages, (unsigned int)(st[DS_PAGE_BUMP] & 0xffffffffu), n_pool, secs, st[DS_ROUNDS], st[DS_CHAINS_RUN], st[DS_CHAINS_DONE], st[DS_STEPS], st[DS_CAREFUL], st[DS_TAIL_RANK], st[DS_TAIL_TEXT],
			st[DS_MAX_CLK] * 1e-8, st[DS_MAX_ROUNDS], st[DS_SUM_CLK] * 1e-8, st[DS_WAVE_CLK] * 1e-8);
	fprintf(stderr, "[nabwa] kernel D phases (wave-s): pop %.1f, chains %.1f, exact tails %.1f (%llu turns), commit %.1f, hit bookkeeping %.1f; active lanes per chain step %.1f\n",
			st[DS_PH_POP] * 1e-8, st[DS_PH_CHAIN] * 1e-8, st[DS_PH_TAIL] * 1e-8, st[DS_TAIL_TURNS], st[DS_PH_COMMIT] * 1e-8, st[DS_PH_HIT] * 1e-8, st[DS_STEPS] ? (double)st[DS_LANE_STEPS] / (double)st[DS_STEPS] : 0.0);
	fprintf(stderr, "[nabwa] kernel D lane-steps %llu: pruned at the pop %llu, expansions %llu (in key form %llu, on two buckets %llu), records %llu, children stored %llu; key-form tails / hits %llu; expansions without a difference allowed: %llu in key form, %llu on one row, %llu on several\n",
			st[DS_LANE_STEPS], st[DS_PRUNED], st[DS_EXPAND], st[DS_KEY_EXPAND], st[DS_TWO], st[DS_RECORDS], st[DS_CHILDREN], st[DS_KEY_TAIL], st[DS_FORCED_KEY], st[DS_FORCED_ONE], st[DS_FORCED_ROWS]);
	if (hist == 2) {
		fprintf(stderr, "[nabwa] kernel D rounds by width (1, 2, 3-4, 5-8, 9-16, 17-32, 33-64 entries):");
		for (int d = 0; d < DS_HIST2_BINS; ++d) fprintf(stderr, " %llu", st[DS_HIST2_ROUNDS + d]);
		fprintf(stderr, "; their wave-steps:");
		for (int d = 0; d < DS_HIST2_BINS; ++d) fprintf(stderr, " %llu", st[DS_HIST2_STEPS + d]);
		fprintf(stderr, "\n");
	}
	if (hist == 1) for (int h = 0; h < 3; ++h) {
		fprintf(stderr, "[nabwa] kernel D expansions by depth (read symbols consumed), %s:", h == 0 ? "rows, several" : (h == 1 ? "rows, one" : "key form"));
		for (int d = 0; d < DS_HIST1_BINS; ++d) fprintf(stderr, " %llu", st[DS_HIST1 + DS_HIST1_BINS * h + d]);
		fprintf(stderr, "\n");
	}
}

/* NABWA_DEEP_DUMP=<file> (investigations of the work order): per search of the first launch its read, length, max_diff, the width
 * passes' restart classes, what kernel S saw of it (trips, hits) and the rounds kernel D needed -- int32 x 8 per search */
namespace {
struct DeepDump {
	const char *path = getenv("NABWA_DEEP_DUMP");
	std::vector<int32_t> ids, trips, naln;      /* as kernel S left them: the list, and per read of the batch max_ent and n_aln */
	PoolBuf<uint32_t> d_rounds;
};
}

/* before the first launch: what the launch overwrites, and the buffer for the rounds */
static int deep_dump_begin(nabwa_batch *b, unsigned int cur, DeepDump &dd)
{
	dd.ids.resize(cur); dd.trips.resize(b->n); dd.naln.resize(b->n);
	HIP_CHECK(hipStreamSynchronize(b->stream));
	HIP_CHECK(hipMemcpy(dd.ids.data(), b->d_ovf_ids, (size_t)cur * 4, hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(dd.trips.data(), b->d_maxent, (size_t)b->n * 4, hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(dd.naln.data(), b->d_naln, (size_t)b->n * 4, hipMemcpyDeviceToHost));
	HIP_CHECK(dd.d_rounds.get(b->ix, (size_t)cur * 4));
	HIP_CHECK(hipMemsetAsync(dd.d_rounds, 0, (size_t)cur * 4, b->stream));
	return NABWA_OK;
}

/* after it: <file> and <file>.all */
static int deep_dump_write(nabwa_batch *b, const DeepDump &dd)
{
	std::vector<uint32_t> rounds(dd.ids.size());
	std::vector<uint8_t> cls((size_t)b->n * 2), md((size_t)b->n); std::vector<int32_t> lens((size_t)b->n);
	HIP_CHECK(hipMemcpy(rounds.data(), dd.d_rounds, rounds.size() * 4, hipMemcpyDeviceToHost));
	if (b->d_cls) HIP_CHECK(hipMemcpy(cls.data(), b->d_cls, cls.size(), hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(md.data(), b->d_md, md.size(), hipMemcpyDeviceToHost));
	HIP_CHECK(hipMemcpy(lens.data(), b->d_len, lens.size() * 4, hipMemcpyDeviceToHost));
	FILE *f = fopen(dd.path, "wb");
	if (f) {
		for (size_t t = 0; t < dd.ids.size(); ++t) {
			const int32_t r = dd.ids[t];
			const int32_t row[8] = { r, lens[r], (int32_t)md[r], (int32_t)cls[2 * (size_t)r], (int32_t)cls[2 * (size_t)r + 1], dd.trips[r], dd.naln[r], (int32_t)rounds[t] };
			fwrite(row, 4, 8, f);
		}
		fclose(f);
	}
	{	/* <file>.all: per read of the batch its two restart classes and whether kernel S handed it on */
		std::vector<uint8_t> st((size_t)b->n);
		HIP_CHECK(hipMemcpy(st.data(), b->d_status, st.size(), hipMemcpyDeviceToHost));
		FILE *g = fopen((std::string(dd.path) + ".all").c_str(), "wb");
		if (g) { for (int i = 0; i < b->n; ++i) { const uint8_t row[4] = { cls[2 * (size_t)i], cls[2 * (size_t)i + 1], (uint8_t)(st[i] != NABWA_ST_OK), md[i] }; fwrite(row, 1, 4, g); } fclose(g); }
	}
	return NABWA_OK;
}

/* A hit list that outgrew the wide rows: the reference's list grows without bound (bwtgap.c:186-190), so those n_hit searches run
 * again with 16 x the rows, then 256 x ... in a block of their own (NABWA_HIT_GROW steps, NABWA_HIT_GROW_GB at most); a table
 * on the device names the rows of every read resolved that way (status NABWA_ST_GROWN, wide_idx = its slot there). */
static int grow_hit_lists(nabwa_batch *b, const DeepParams &D, unsigned int n_hit, long n_waves, bool timing)
{
	size_t cap3 = (size_t)b->aln_cap2;
	for (int grow = 0; n_hit && grow < env_int("NABWA_HIT_GROW", 3) && b->n_grown < 8; ++grow) {
		cap3 *= 16;
		const size_t bytes = (size_t)n_hit * cap3 * 16;
		if (bytes > ((size_t)env_int("NABWA_HIT_GROW_GB", 8) << 30) || cap3 > 0x7fffffffu) break;
		PoolBuf<int32_t> n3, m3; PoolBuf<uint8_t> s3;
		StreamDrain drain{ b->stream };
		HIP_CHECK(b->grown[b->n_grown].get(b->ix, bytes));
		uint8_t *const base = b->grown[b->n_grown++];
		HIP_CHECK(n3.get(b->ix, (size_t)n_hit * 4)); HIP_CHECK(m3.get(b->ix, (size_t)n_hit * 4)); HIP_CHECK(s3.get(b->ix, n_hit));
		if (!b->d_grown_tab || (b->grown_used == 0 && b->grown_cap < 8 * (int)n_hit + 8)) {      /* every step resolves or repeats reads of the first step's list */
			if (b->d_grown_tab) { HIP_CHECK(hipStreamSynchronize(b->stream)); HIP_CHECK(b->d_grown_tab.release()); }
			b->grown_cap = 8 * (int)n_hit + 8;
			HIP_CHECK(b->d_grown_tab.get(b->ix, (size_t)b->grown_cap * 8));
			b->grown_used = 0;
		}
		if (b->grown_used + (int)n_hit > b->grown_cap) break;
		DeepParams G = D;
		G.S.res_slot = 0; G.S.n_aln = n3; G.S.max_ent = m3; G.S.status = s3; G.S.aln = (uint4*)base; G.S.aln_cap = (int)cap3;
		G.rounds_out = 0;
		long waves = (long)(b->deep_n_pages / b->deep_cap_pages);          /* as many searches at a time as the pool can hold in the worst case */
		if (waves < 1) waves = 1;
		if (waves > n_waves) waves = n_waves;
		if (waves > (long)n_hit) waves = (long)n_hit;
		const unsigned int n_again = n_hit;
		if (int r = deep_launch(b, G, n_again, waves, false, &n_hit)) return r;
		HIP_CHECK(n3.release()); HIP_CHECK(m3.release()); HIP_CHECK(s3.release());
		if (timing) fprintf(stderr, "[nabwa] kernel D, hit lists beyond %d rows: %u reads searched again with %zu rows each\n", b->aln_cap2, n_again, cap3);
	}
	b->unresolved = (int)n_hit;
	if (n_hit) return nabwa_fail(NABWA_EHITS, "reads with more hit rows than the grown lists hold (NABWA_ALNCAP2 x 16^NABWA_HIT_GROW within NABWA_HIT_GROW_GB): their n_aln is reported as 0, every other read is resolved");
	return NABWA_OK;
}

/* kernel D over the `cur` reads of d_ovf_ids: run it, see what is left, run the guaranteed pass, grow the hit lists */
int deep_searches(nabwa_batch *b, unsigned int cur, bool timing)
{
	/* a chain's matching child must be the only child of its own score (fm_deep_body.hpp) */
	if (b->opt.s_mm < 1 || b->opt.s_gapo < 1 || b->opt.s_gape < 1) return nabwa_fail(NABWA_EINVAL, "deep searches need s_mm, s_gapo, s_gape >= 1");
	const double tt0 = now_s();
	if (int r = grow_wide_rows(b, cur)) return r;
	nabwa_launch_assign_slots((int)cur, b->d_ovf_ids, b->d_wide_idx, b->stream);
	if (!b->deep_cfg) if (int r = deep_configure(b)) return r;
	const size_t n_pages = b->deep_n_pages; const uint64_t cap_pages = b->deep_cap_pages;
	long n_waves = b->deep_waves_max;
	if (n_waves > (long)cur) n_waves = (long)cur;
	if (int r = deep_grow_buffers(b, n_waves)) return r;
	DeepDump dump;
	StreamDrain drain{ b->stream };
	DeepParams D;
	deep_fill_params(b, D, timing || getenv("NABWA_DEEP_STATS") || dump.path);
	if (dump.path) {
		if (int r = deep_dump_begin(b, cur, dump)) return r;
		D.rounds_out = dump.d_rounds;
	}
	// pass 1: as many waves as fit the CUs, pages on demand; pass 2 (only if the pool ran dry under some reads): as many
	// waves as the pool can serve in the worst case
	unsigned int todo = cur, n_pool = 0;
	for (int pass = 0; pass < 2 && todo; ++pass) {
		long waves = n_waves;
		if (pass == 1) {
			waves = (long)(n_pages / cap_pages);
			if (waves < 1) waves = 1;
			if (waves > n_waves) waves = n_waves;
		}
		if (waves > (long)todo) waves = (long)todo;
		if (int r = deep_launch(b, D, todo, waves, pass == 0, &n_pool)) return r;
		if (timing) {
			unsigned long long st[DS_WORDS];
			HIP_CHECK(hipMemcpy(st, b->d_deep_ctr, sizeof st, hipMemcpyDeviceToHost));
			deep_print_stats(st, env_int("NABWA_DEEP_HIST", 0), pass == 1, todo, waves, n_pages, n_pool, now_s() - tt0);
		}
		if (pass == 0 && dump.path) {
			if (int r = deep_dump_write(b, dump)) return r;
			HIP_CHECK(dump.d_rounds.release()); D.rounds_out = 0;
		}
		todo = n_pool;
	}
	b->deep_ran = 1;
	HIP_CHECK(hipEventElapsedTime(&b->last_ms_deep, b->evd0, b->evd1));
	if (todo) { b->unresolved = (int)todo; return nabwa_fail(NABWA_ENOMEM, "kernel D: the page pool cannot hold one worst-case search (raise NABWA_DEEP_GB or lower max_entries)"); }
	unsigned int n_hit = 0;
	if (int r = recollect(b, NABWA_ST_HITCAP, &n_hit)) return r;
	return grow_hit_lists(b, D, n_hit, n_waves, timing);
}
