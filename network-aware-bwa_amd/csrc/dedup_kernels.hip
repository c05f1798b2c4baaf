// dedup_kernels.hip -- the kernels of the duplicate-read stage of a search batch (gfx950; NABWA_DEDUP=1, nabwa_batch.hip: dedup_reads):
// hash every read, and -- after the host's radix sort of (hash, read) and its scan of the run starts -- compare every read with the first
// read of its run, number the representatives, and copy their bytes into compact raw buffers.  On the way out (nabwa_batch_fetch) the
// counts of the caller's reads are taken through the map.  The bodies are in dedup_body.hpp.
#include "nabwa_dev.hpp"
#include "dedup_cache_body.hpp"
#include "launchers.hpp"

// 16 lanes per read (one thread per read walking bytes: 62 ms for 10 M reads, pad_reads_kernel).  keys[i] = the low bits of read i's hash
// that `mask` keeps, ids[i] = i: the pairs the sort takes.
__global__ __launch_bounds__(256) void dedup_hash_kernel(int n, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq,
														 const int64_t *__restrict__ off, uint64_t mask, uint64_t *__restrict__ keys, uint32_t *__restrict__ ids)
{
	const int t = threadIdx.x & 15;
	const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
	if (i >= n) return;                                          /* whole 16-lane groups leave together */
	const int64_t o = off[i];
	const int L = (int)(off[i + 1] - o);
	uint64_t sum = dedup_hash_part(seq, rseq, o, L, t);
	for (int m = 8; m; m >>= 1) sum += __shfl_xor(sum, m, 16);
	if (t == 0) { keys[i] = dedup_hash_finish(sum, L) & mask; ids[i] = (uint32_t)i; }
}

// head[j] = j where a run of equal keys starts in the sorted order, else 0: an inclusive max-scan then gives every position its run's start
__global__ __launch_bounds__(256) void dedup_heads_kernel(int n, const uint64_t *__restrict__ keys, uint32_t *__restrict__ head)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j < n) head[j] = j > 0 && keys[j] != keys[j - 1] ? (uint32_t)j : 0u;
}

// sorted position j: read ids[j] against the first read of its run, ids[head[j]] (the sort is stable: the smallest id of the run).  Equal
// bytes and length: that read represents it.  Otherwise the hash collided: the read represents itself and is counted.  flag[i] = 1 for
// the representatives, and flag[n] = 0 closes the scan that numbers them.
__global__ __launch_bounds__(256) void dedup_verify_kernel(int n, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq,
														   const int64_t *__restrict__ off, const uint32_t *__restrict__ ids, const uint32_t *__restrict__ head,
														   int32_t *__restrict__ rep, uint32_t *__restrict__ flag, unsigned int *__restrict__ n_coll)
{
	const int t = threadIdx.x & 15;
	const int j = blockIdx.x * 16 + (threadIdx.x >> 4);
	if (j >= n) return;
	if (j == 0 && t == 0) flag[n] = 0u;
	const int i = (int)ids[j], f = (int)ids[head[j]];
	const int64_t oa = off[i], ob = off[f];
	const int L = (int)(off[i + 1] - oa);
	int same = f == i || L == (int)(off[f + 1] - ob) ? 1 : 0;
	if (f != i && same) same = dedup_equal_part(seq, rseq, oa, ob, L, t) ? 1 : 0;
	for (int m = 8; m; m >>= 1) same &= __shfl_xor(same, m, 16);
	if (t == 0) {
		rep[i] = same ? f : i; flag[i] = same && f != i ? 0u : 1u;
		if (!same) atomicAdd(n_coll, 1u);
	}
}

// inner[i]: the representatives before read i (exclusive sum of flag; inner[n] = their number).  map[i] = the inner index of read i's
// representative; a representative also enters its length for the scan that gives the compact starts (clen[n_u] = 0 closes it), and
// stat[1] = n_u goes to the host with stat[0], the collisions.
__global__ __launch_bounds__(256) void dedup_map_kernel(int n, const int32_t *__restrict__ rep, const uint32_t *__restrict__ inner,
														const int64_t *__restrict__ off, int32_t *__restrict__ map, int64_t *__restrict__ clen, unsigned int *__restrict__ stat)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i > n) return;
	if (i == n) { clen[inner[n]] = 0; stat[1] = inner[n]; return; }
	const int r = rep[i];
	map[i] = (int32_t)inner[r];
	if (r == i) clen[inner[i]] = off[i + 1] - off[i];
}

// the representatives' bytes, both strands, back to back in the caller's order: read i -> compact read inner[i] at coff[inner[i]].
// 16 lanes per read, a 16-byte chunk per lane and turn; source and destination start at any byte, the tail goes byte-wise.  coff[n_u] is
// the compact total (at most off[n]): nothing is written at or beyond it.
__global__ __launch_bounds__(256) void dedup_compact_kernel(int n, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq,
															const int64_t *__restrict__ off, const int32_t *__restrict__ rep, const uint32_t *__restrict__ inner,
															const int64_t *__restrict__ coff, uint8_t *__restrict__ cseq, uint8_t *__restrict__ crseq)
{
	const int t = threadIdx.x & 15;
	const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
	if (i >= n || rep[i] != i) return;
	const int64_t o = off[i], d = coff[inner[i]];
	const int L = (int)(off[i + 1] - o), NC = (L + 15) >> 4;
	for (int c = t; c < NC; c += 16) {
		const int have = L - 16 * c;
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			const uint8_t *src = (st ? rseq : seq) + o + 16 * (int64_t)c;
			uint8_t *dst = (st ? crseq : cseq) + d + 16 * (int64_t)c;
			if (have >= 16) { uint32_t w[4]; __builtin_memcpy(w, src, 16); __builtin_memcpy(dst, w, 16); }
			else for (int k = 0; k < have; ++k) dst[k] = src[k];
		}
	}
}

// the counts and max_entries of the caller's reads: those of the reads searched, through the map; a negative map value -1 - k names served
// read k, whose entry lies at arena + 16 * cent[k] (NABWA_DEDUP_CACHE, dedup_cache_body.hpp)
__global__ __launch_bounds__(256) void dedup_expand_kernel(int n, const int32_t *__restrict__ map, const int32_t *__restrict__ n_aln, const int32_t *__restrict__ max_ent,
														   const uint32_t *__restrict__ cent, const uint8_t *__restrict__ arena,
														   int32_t *__restrict__ n_aln_out, int32_t *__restrict__ max_ent_out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int s = map[i];
	if (s >= 0) { n_aln_out[i] = n_aln[s]; max_ent_out[i] = max_ent[s]; }
	else { const uint8_t *e = arena + (size_t)cent[-1 - s] * 16; n_aln_out[i] = dcache_n_aln(e); max_ent_out[i] = dcache_max_ent(e); }
}

extern "C" void nabwa_launch_dedup_hash(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, uint64_t mask, uint64_t *keys, uint32_t *ids, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dedup_hash_kernel, dim3((n + 15) / 16), dim3(256), 0, s, n, seq, rseq, off, mask, keys, ids);
}

extern "C" void nabwa_launch_dedup_heads(int n, const uint64_t *keys, uint32_t *head, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dedup_heads_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, keys, head);
}

extern "C" void nabwa_launch_dedup_verify(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const uint32_t *ids, const uint32_t *head,
										  int32_t *rep, uint32_t *flag, unsigned int *n_coll, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dedup_verify_kernel, dim3((n + 15) / 16), dim3(256), 0, s, n, seq, rseq, off, ids, head, rep, flag, n_coll);
}

extern "C" void nabwa_launch_dedup_map(int n, const int32_t *rep, const uint32_t *inner, const int64_t *off, int32_t *map, int64_t *clen, unsigned int *stat, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dedup_map_kernel, dim3(n / 256 + 1), dim3(256), 0, s, n, rep, inner, off, map, clen, stat);
}

extern "C" void nabwa_launch_dedup_compact(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const int32_t *rep, const uint32_t *inner,
										   const int64_t *coff, uint8_t *cseq, uint8_t *crseq, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dedup_compact_kernel, dim3((n + 15) / 16), dim3(256), 0, s, n, seq, rseq, off, rep, inner, coff, cseq, crseq);
}

extern "C" void nabwa_launch_dedup_expand(int n, const int32_t *map, const int32_t *n_aln, const int32_t *max_ent, const uint32_t *cent, const uint8_t *arena,
										  int32_t *n_aln_out, int32_t *max_ent_out, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(dedup_expand_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, map, n_aln, max_ent, cent, arena, n_aln_out, max_ent_out);
}
