// dedup_cache_kernels.hip -- the kernels of the cross-batch read cache (gfx950; NABWA_DEDUP_CACHE, nabwa_batch.hip: cache_lookup and
// cache_insert).  Lookup, over the distinct reads NABWA_DEDUP=1 leaves of a batch: probe the table, compare the candidates byte for byte,
// number the reads that still need a search and those an entry serves, and rewrite the batch's map.  Insert, over the reads searched once
// their results are final: claim a slot, reserve arena bytes, write the entry.  The bodies are in dedup_cache_body.hpp.
#include "nabwa_dev.hpp"
#include "fm_search.hpp"
#include "dedup_cache_body.hpp"
#include "launchers.hpp"

// 16 lanes per read, as dedup_verify_kernel.  found[i] = the arena offset / 16 + 1 of the entry that answers for read i, or 0; flag[i] = 1 for
// the reads to search and flag[n] = 0 closes the scan that numbers them.  The 16 lanes of a read load the same slots and header words, so
// they take every branch together and the shuffles below only ever read lanes that are running.
__global__ __launch_bounds__(256) void dcache_lookup_kernel(int n, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq, const int64_t *__restrict__ off,
															const uint64_t *__restrict__ hash, const uint8_t *__restrict__ md_tab, const uint8_t *__restrict__ mg_tab,
															const unsigned long long *__restrict__ slots, uint32_t n_slots, uint64_t mask,
															const uint8_t *__restrict__ arena, uint32_t *__restrict__ found, uint32_t *__restrict__ flag)
{
	const int t = threadIdx.x & 15;
	const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
	if (i >= n) return;                                          /* whole 16-lane groups leave together */
	if (i == 0 && t == 0) flag[n] = 0u;
	const int64_t o = off[i];
	const int L = (int)(off[i + 1] - o);
	const uint64_t h = hash[i];
	const int md = md_tab[L], mg = mg_tab[L];
	uint32_t hit = 0;
	int p = 0;
	for (;;) {
		const uint64_t cand = dcache_next_candidate(slots, n_slots, h, mask, &p);
		if (!cand) break;
		int same = dcache_match_part(arena + (cand - 1) * 16, h, seq, rseq, o, L, md, mg, t) ? 1 : 0;
		for (int m = 8; m; m >>= 1) same &= __shfl_xor(same, m, 16);
		if (same) { hit = (uint32_t)cand; break; }
	}
	if (t == 0) { found[i] = hit; flag[i] = hit ? 0u : 1u; }
}

// inner[i]: the reads to search before read i (inner[n]: their number n_s).  A read to search: rep[i] = i, newidx[i] = inner[i] and its
// length enters the scan of the compact starts (clen[n_s] = 0 closes it).  A served read: rep[i] = -1 (dedup_compact_kernel passes over
// it), it is served read k = i - inner[i], cent[k] = its entry's arena offset / 16, newidx[i] = -1 - k.  stat[0] = n_s.
__global__ __launch_bounds__(256) void dcache_map_kernel(int n, const uint32_t *__restrict__ found, const uint32_t *__restrict__ inner, const int64_t *__restrict__ off,
														 int32_t *__restrict__ rep, int32_t *__restrict__ newidx, int64_t *__restrict__ clen, uint32_t *__restrict__ cent,
														 unsigned int *__restrict__ stat)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	if (i == n) { clen[inner[n]] = 0; stat[0] = inner[n]; return; }
	const uint32_t f = found[i];
	if (f) { const uint32_t k = (uint32_t)i - inner[i]; rep[i] = -1; cent[k] = f - 1u; newidx[i] = -1 - (int32_t)k; }
	else { rep[i] = i; newidx[i] = (int32_t)inner[i]; clen[inner[i]] = off[i + 1] - off[i]; }
}

// the caller's read j -> the distinct read old[j] (null: j itself) -> newidx: a read searched (>= 0) or served read -1 - value
__global__ __launch_bounds__(256) void dcache_remap_kernel(int n, const int32_t *__restrict__ old, const int32_t *__restrict__ newidx, int32_t *__restrict__ map)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j < n) map[j] = newidx[old ? old[j] : j];
}

// 16 lanes per read searched, over the batch's padded reads (16-byte aligned starts; only the read's own bytes are read).  Lane 0 decides:
// a complete search (not handed on, not cut short) of at most row_cap rows claims a slot, then reserves the entry's bytes; a slot whose
// reserve fails stays DCACHE_CLAIMED.  Then the 16 lanes write the entry and lane 0 publishes the slot.  The hash is computed here again:
// it depends on the bytes and the length alone, not on where the read lies.
__global__ __launch_bounds__(256) void dcache_insert_kernel(int n, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq, const int64_t *__restrict__ poff,
															const int32_t *__restrict__ len, const uint8_t *__restrict__ rd_md, const uint8_t *__restrict__ rd_mg,
															const uint8_t *__restrict__ status, const int32_t *__restrict__ n_aln, const int32_t *__restrict__ max_ent,
															const uint4 *__restrict__ aln, int aln_cap, const int32_t *__restrict__ wide_idx, const uint4 *__restrict__ aln2, int aln_cap2,
															const uint4 *const *__restrict__ grown, int row_cap, uint64_t mask,
															unsigned long long *__restrict__ slots, uint32_t n_slots, uint8_t *__restrict__ arena, uint64_t arena_bytes,
															unsigned long long *__restrict__ ctr)
{
	const int t = threadIdx.x & 15;
	const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
	if (i >= n) return;
	const int64_t o = poff[i];
	const int L = len[i];
	uint64_t sum = dedup_hash_part(seq, rseq, o, L, t);
	for (int m = 8; m; m >>= 1) sum += __shfl_xor(sum, m, 16);
	const uint64_t h = dedup_hash_finish(sum, L);
	const int st = status[i], na = n_aln[i];
	long long where = -1;      /* the entry's arena offset, a multiple of 16 */
	int64_t slot = -1;
	if (t == 0) {
		const bool complete = st == NABWA_ST_OK || st == NABWA_ST_WIDE || st == NABWA_ST_GROWN;
		where = dcache_insert_claim(slots, n_slots, h, mask, ctr, arena_bytes, L, na, complete && na >= 0 && na <= row_cap, &slot);
	}
	where = __shfl(where, 0, 16);      /* lane 0's decision to the read's 16 lanes */
	if (where < 0) return;
	const uint4 *rows = st == NABWA_ST_GROWN ? grown[wide_idx[i]] : st == NABWA_ST_WIDE ? aln2 + (size_t)wide_idx[i] * aln_cap2 : aln + (size_t)i * aln_cap;
	dcache_write_part(arena + where, h, seq, rseq, o, L, rd_md[i], rd_mg[i], na, max_ent[i], rows, t);
	if (t == 0) dcache_store(slots + slot, dcache_slot_value(h, (uint64_t)where >> 4));
}

extern "C" void nabwa_launch_dcache_lookup(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const uint64_t *hash, const uint8_t *md_tab, const uint8_t *mg_tab,
										   const unsigned long long *slots, uint32_t n_slots, uint64_t mask, const uint8_t *arena, uint32_t *found, uint32_t *flag, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dcache_lookup_kernel, dim3((n + 15) / 16), dim3(256), 0, s, n, seq, rseq, off, hash, md_tab, mg_tab, slots, n_slots, mask, arena, found, flag);
}

extern "C" void nabwa_launch_dcache_map(int n, const uint32_t *found, const uint32_t *inner, const int64_t *off, int32_t *rep, int32_t *newidx, int64_t *clen, uint32_t *cent,
										unsigned int *stat, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dcache_map_kernel, dim3(n / 256 + 1), dim3(256), 0, s, n, found, inner, off, rep, newidx, clen, cent, stat);
}

extern "C" void nabwa_launch_dcache_remap(int n, const int32_t *old, const int32_t *newidx, int32_t *map, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dcache_remap_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, old, newidx, map);
}

extern "C" void nabwa_launch_dcache_insert(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *poff, const int32_t *len, const uint8_t *rd_md, const uint8_t *rd_mg,
										   const uint8_t *status, const int32_t *n_aln, const int32_t *max_ent, const uint4 *aln, int aln_cap, const int32_t *wide_idx,
										   const uint4 *aln2, int aln_cap2, const uint4 *const *grown, int row_cap, uint64_t mask,
										   unsigned long long *slots, uint32_t n_slots, uint8_t *arena, uint64_t arena_bytes, unsigned long long *ctr, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dcache_insert_kernel, dim3((n + 15) / 16), dim3(256), 0, s, n, seq, rseq, poff, len, rd_md, rd_mg, status, n_aln, max_ent, aln, aln_cap, wide_idx,
					   aln2, aln_cap2, grown, row_cap, mask, slots, n_slots, arena, arena_bytes, ctr);
}
