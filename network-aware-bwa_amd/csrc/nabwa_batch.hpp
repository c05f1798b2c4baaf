// nabwa_batch.hpp -- the search batch as its two units see it: nabwa_batch.hip (the nabwa_batch_* entries, kernels W and S) and
// nabwa_batch_deep.hip (the host side of kernel D, which nabwa_batch_sync hands the flagged reads to).
#pragma once
#include "launchers.hpp"
#include "dev_pool.hpp"

#pragma GCC visibility push(hidden)

/* Every device buffer, event and stream is a handle (dev_pool.hpp): deleting the batch returns them.  The stream comes first so that
 * it goes last. */
struct nabwa_batch {
	nabwa_index *ix = nullptr;
	nabwa_gap_opt_t opt = {};
	int n = 0;                       // the reads searched: what every kernel and buffer of the search counts by
	/* NABWA_DEDUP=1 (nabwa_batch.hip: dedup_reads): n_given is the caller's count, n the distinct reads among them; d_map, when held, takes
	 * a caller's read to the read searched for it (n_given entries).  No map: n == n_given and the batch is what it is without the switch */
	int n_given = 0, dedup_on = 0; unsigned int dedup_coll = 0;
	DevStream stream;
	DevEvent ev0, ev1, evw;
	float last_ms = 0.f;
	// device inputs
	PoolBuf<uint8_t> d_seq, d_rseq, d_md, d_mg; PoolBuf<int64_t> d_poff; PoolBuf<int32_t> d_len; PoolBuf<uint32_t> d_key, d_pack; int pack_stride = 0;
	PoolBuf<int32_t> d_map;
	/* NABWA_DEDUP_CACHE (nabwa_batch.hip: cache_lookup, cache_insert): cache is the index's read cache while this batch looks up in it and
	 * inserts into it (null: off, or bypassed).  n_served of the distinct reads were found there and are not searched: n counts the others, a
	 * d_map value -1 - k stands for served read k, and d_cent[k] is its entry's arena offset / 16.  A batch with served reads pins the cache
	 * until it is destroyed.  cache_mask: the probe key's bits (NABWA_DEDUP_HASH_BITS) */
	nabwa_dedup_cache *cache = nullptr; uint64_t cache_sig = 0, cache_mask = ~0ull;
	int cache_on = 0, cache_bypass = 0, cache_pinned = 0, cache_inserted = 0, n_served = 0;
	uint64_t n_inserted = 0, n_not_inserted = 0; float cache_lookup_ms = 0.f, cache_insert_ms = 0.f;
	PoolBuf<uint32_t> d_cent;
	PoolBuf<unsigned long long> d_s0stats; PoolBuf<uint8_t> d_cls; PoolBuf<int32_t> d_perm; PoolBuf<unsigned int> d_ncls; int max_len = 0;
	// first pass
	SearchParams P = {}; int class_sort = 0; uint32_t NS_wide = 0; int n_blocks = 0, n_blocks_w = 0; PoolBuf<uint8_t> d_scratch, d_wdata, d_nN; float last_ms_w = 0.f;
	PoolBuf<int32_t> d_naln, d_maxent, d_wide_idx; PoolBuf<uint8_t> d_status; PoolBuf<uint4> d_aln;
	PoolBuf<unsigned int> d_counter, d_novf; PoolBuf<int32_t> d_ovf_ids;
	PoolBuf<uint8_t> grown[8]; int n_grown = 0;           // row blocks of the reads whose hit lists outgrew the wide rows (nabwa_batch_sync)
	PoolBuf<const uint4*> d_grown_tab; int grown_cap = 0, grown_used = 0;      // device table: slot -> rows of one such read (wide_idx of a NABWA_ST_GROWN read)
	// wide pass (allocated on demand)
	int n2 = 0, aln_cap2 = 0; PoolBuf<uint8_t> d_scratch2; size_t scratch2_bytes = 0; PoolBuf<int32_t> d_naln2, d_maxent2; PoolBuf<uint8_t> d_status2; PoolBuf<uint4> d_aln2;
	int unresolved = 0;
	int w_stats_armed = 0; unsigned long long w_stats[6] = { 0, 0, 0, 0, 0, 0 };      /* NABWA_W_STATS: slots TS_W_TRIPS .. TS_W_STEP of kernel W's last launch with statistics */
	PoolBuf<unsigned long long> d_sum;
	// kernel D (deep searches): page pool, per-wave page lists and staging, counters; allocated on demand, kept for the next run
	PoolBuf<uint4> d_pages; PoolBuf<uint32_t> d_page_prev, d_deep_own; PoolBuf<uint4> d_deep_stage; PoolBuf<unsigned long long> d_deep_ctr;
	PoolBuf<uint32_t> d_ixtab;
	size_t deep_pages = 0, deep_own_words = 0, deep_stage_ent = 0;
	DevEvent evd0, evd1; float last_ms_deep = 0.f; int deep_ran = 0, deep_only = 0;
	int deep_cfg = 0; uint32_t deep_K = 0, deep_lds_rd = 0, deep_rd_pl = 0; size_t deep_n_pages = 0; uint64_t deep_cap_pages = 0; long deep_waves_max = 0;
	// what nabwa_batch_config reports and nothing reads back otherwise
	int min_len = 0, ran = 0, deep_coop = 0; uint32_t NS1 = 0;
};

static inline uint32_t align_up(uint32_t x, uint32_t a) { return (x + a - 1) / a * a; }

/* nabwa_batch.hip */
void rebuild_widths(nabwa_batch *b, const SearchParams &Q, unsigned int cnt, bool after_first_pass);
int recollect(nabwa_batch *b, int which, unsigned int *left);
/* nabwa_batch_deep.hip */
int deep_searches(nabwa_batch *b, unsigned int cur, bool timing);

#pragma GCC visibility pop
