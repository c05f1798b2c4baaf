// batch_kernels.hip -- the small kernels a batch runs around its searches (gfx950): the re-layout of the reads, the work order by
// class, the lists of reads handed on, the scatter of their results, row compaction and the checksum.
#include "nabwa_dev.hpp"
#include "fm_search.hpp"
#include "dedup_cache_body.hpp"
#include "launchers.hpp"

// re-lay the reads out with every read starting on a 16-byte boundary (register windows load 16 bases), and form
// the interval-table keys: the first T symbols the search consumes (positions len-1 down to len-T) of each strand.
// 16 lanes per read, one 16-base chunk of both strands per lane and turn: loads and stores of a read are consecutive
// across its lanes (one thread per read walking bytes took 62 ms for 10 M reads; this form streams at HBM rate).
__global__ __launch_bounds__(256) void pad_reads_kernel(int n, const uint8_t *__restrict__ seq, const uint8_t *__restrict__ rseq,
													const int64_t *__restrict__ off, const int64_t *__restrict__ poff,
													uint8_t *__restrict__ pseq, uint8_t *__restrict__ prseq, int32_t *__restrict__ rd_len,
													uint32_t *__restrict__ rd_key, int T, int seed_len, uint32_t *__restrict__ rd_pack, int pack_stride,
													const uint8_t *__restrict__ md_tab, const uint8_t *__restrict__ mg_tab,
													uint8_t *__restrict__ rd_md, uint8_t *__restrict__ rd_mg)
{
	const int t = threadIdx.x & 15;
	const int i = blockIdx.x * 16 + (threadIdx.x >> 4);
	if (i >= n) return;                                          /* whole 16-lane groups leave together */
	const int64_t o = off[i], p = poff[i];
	const int L = (int)(off[i + 1] - o), NC = (int)(poff[i + 1] - p) >> 4;
	if (t == 0) { rd_len[i] = L; rd_md[i] = md_tab[L]; rd_mg[i] = mg_tab[L]; }      /* max_diff / max_gapo of a read follow from its length (host tables) */
	// both strands 2 bits per base as well, base j in word j>>4 from the TOP bits down, so that the 16 symbols from any position
	// are one 32-bit extract in table-key order; the word after the last says whether the strand holds an N (then: no keys)
	const int PW = pack_stride / 2;
	uint32_t *const pk = rd_pack ? rd_pack + (size_t)i * pack_stride : 0;
	const int n_turns = pk && PW - 1 > NC ? PW - 1 : NC;
	uint32_t anyN[2] = { 0u, 0u };
	for (int c = t; c < n_turns; c += 16) {
		for (int st = 0; st < 2; ++st) {
			const uint8_t *src = (st ? rseq : seq) + o + 16 * c;
			uint32_t w[4] = { 0x04040404u, 0x04040404u, 0x04040404u, 0x04040404u };
			const int have = L - 16 * c;                          /* bases of this chunk that exist */
			if (have >= 16) __builtin_memcpy(w, src, 16);
			else {
#pragma unroll
				for (int k = 0; k < 16; ++k) if (k < have) { const uint32_t v = src[k]; w[k >> 2] = (w[k >> 2] & ~(0xffu << (8 * (k & 3)))) | v << (8 * (k & 3)); }
			}
			if (c < NC) *(uint4*)((st ? prseq : pseq) + p + 16 * c) = make_uint4(w[0], w[1], w[2], w[3]);
			if (pk && c < PW - 1) {
				uint32_t x = 0;
#pragma unroll
				for (int k = 0; k < 16; ++k) {
					const uint32_t v = k < have ? (w[k >> 2] >> (8 * (k & 3)) & 0xffu) : 0u;
					anyN[st] |= v > 3u ? 1u : 0u;
					x |= (v & 3u) << (30 - 2 * k);
				}
				pk[st * PW + c] = x;
			}
		}
	}
	if (pk) {
		for (int m = 8; m; m >>= 1) { anyN[0] |= __shfl_xor(anyN[0], m, 16); anyN[1] |= __shfl_xor(anyN[1], m, 16); }
		if (t < 2) pk[t * PW + PW - 1] = anyN[t];
	}
	// keys (first consumed symbol = most significant digit): [0,1] kernel S, from position L-1 downwards, seq / rseq;
	// [2,3] kernel W full passes, from position 0 upwards; [4,5] kernel W seed passes, from position L-seed_len upwards
	if (t < 6) {
		const int v = t >> 1;
		uint32_t key = 0xffffffffu;
		if (T > 0 && L > T && (v < 2 || (L > seed_len && seed_len > T))) {
			const uint8_t *src = ((t & 1) ? rseq : seq) + o;
			uint32_t a = 0; bool ok = true;
			for (int q = 1; q <= T; ++q) {
				const int pos = v == 0 ? L - q : (v == 1 ? q - 1 : L - seed_len + q - 1);
				const uint32_t x = src[pos];
				ok = ok && x < 4u; a = a << 2 | (x & 3u);
			}
			if (ok) key = a;
		}
		rd_key[6 * (size_t)i + t] = key;
	}
}

extern "C" void nabwa_launch_pad_reads(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const int64_t *poff,
									   uint8_t *pseq, uint8_t *prseq, int32_t *rd_len, uint32_t *rd_key, int T, int seed_len, uint32_t *rd_pack, int pack_stride,
									   const uint8_t *md_tab, const uint8_t *mg_tab, uint8_t *rd_md, uint8_t *rd_mg, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(pad_reads_kernel, dim3((n + 15) / 16), dim3(256), 0, s, n, seq, rseq, off, poff, pseq, prseq, rd_len, rd_key, T, seed_len, rd_pack, pack_stride,
					   md_tab, mg_tab, rd_md, rd_mg);
}

// padded length of every read (starts go on 16-byte boundaries), and 0 after the last: input of the scan that gives the starts
__global__ __launch_bounds__(256) void padded_len_kernel(int n, const int64_t *__restrict__ off, int64_t *__restrict__ plen)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i <= n) plen[i] = i < n ? (off[i + 1] - off[i] + 15) / 16 * 16 : 0;
}

extern "C" void nabwa_launch_padded_len(int n, const int64_t *off, int64_t *plen, hipStream_t s)
{
	hipLaunchKernelGGL(padded_len_kernel, dim3(n / 256 + 1), dim3(256), 0, s, n, off, plen);
}

__global__ __launch_bounds__(256) void collect_kernel(int n, const uint8_t *__restrict__ status, int32_t *__restrict__ ids,
												  unsigned int *__restrict__ count, int which)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i < n && status[i] == which) ids[atomicAdd(count, 1u)] = i;
}

// The same, in the order kernel D should start them: its launch ends with its longest search, so the searches that look
// longest go first.  (Measured with NABWA_DEEP_DUMP + profiles/probes/deep_order_probe.py on the ancient-DNA workload: by the searches'
// round counts this key schedules no better than a random order, 1.19 x the bound, and a key of {no hit yet, max_diff, read length}
// reaches 1.07 -- but the launch got 4 % SLOWER with it: the longest search then runs its whole life beside a full machine, 21 us per
// round instead of 17 when it finishes alone.  Wave priority for the head of the list changed nothing.  Not kept.)  Key = max_diff - (the lower bound of the read's differences from kernel W: the smaller restart count of
// its two strands): the more differences the bounds leave open, the larger the tree; reads that filled the first pass's hit list
// (repeat families: hundreds of hit rows, every one-difference variant walked to the end) go before everything else.  One pass per
// key value, largest first.
__global__ __launch_bounds__(256) void collect_keyed_kernel(int n, const uint8_t *__restrict__ status, int32_t *__restrict__ ids,
															unsigned int *__restrict__ count, int which, const uint8_t *__restrict__ cls,
															const uint8_t *__restrict__ md, int lo, int hi, const int32_t *__restrict__ n_aln, int aln_cap, int max_key)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n || status[i] != which) return;
	const int c0 = cls[2 * (size_t)i], c1 = cls[2 * (size_t)i + 1];
	int k = (int)md[i] - (c0 < c1 ? c0 : c1);
	if (n_aln[i] >= aln_cap) k = max_key;          // the first pass filled its hit list: a read from a repeat family, the longest searches there are
	if (k >= lo && k <= hi) ids[atomicAdd(count, 1u)] = i;
}

extern "C" void nabwa_launch_collect_keyed(int n, const uint8_t *status, int32_t *ids, unsigned int *count, int which,
										   const uint8_t *cls, const uint8_t *md, int max_key, const int32_t *n_aln, int aln_cap, hipStream_t s)
{
	if (n <= 0) return;
	for (int key = max_key; key >= 0; --key)
		hipLaunchKernelGGL(collect_keyed_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, status, ids, count, which, cls, md,
						   key ? key : -0x7fffffff, key == max_key ? 0x7fffffff : key, n_aln, aln_cap, max_key);
}

// ids of the reads whose status is `which` (NABWA_ST_OVERFLOW after kernel S, NABWA_ST_POOL / NABWA_ST_HITCAP after kernel D)
extern "C" void nabwa_launch_collect(int n, const uint8_t *status, int32_t *ids, unsigned int *count, int which, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(collect_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, status, ids, count, which);
}

__global__ __launch_bounds__(256) void scatter_wide_kernel(int n2, const int32_t *__restrict__ ids, const int32_t *__restrict__ n_aln2,
													   const int32_t *__restrict__ max_ent2, const uint8_t *__restrict__ status2,
													   int32_t *__restrict__ n_aln, int32_t *__restrict__ max_ent,
													   uint8_t *__restrict__ status, const int32_t *__restrict__ wide_idx)
{
	const int q = blockIdx.x * 256 + threadIdx.x;
	if (q >= n2) return;
	const int rid = ids[q], j = wide_idx[rid];       /* j: the read's row in the wide result arrays (assign_slots_kernel) */
	if (status2[j] == NABWA_ST_OK) { n_aln[rid] = n_aln2[j]; max_ent[rid] = max_ent2[j]; status[rid] = NABWA_ST_WIDE; }
	else { n_aln[rid] = 0; max_ent[rid] = max_ent2[j]; status[rid] = status2[j]; }     /* NABWA_ST_POOL / NABWA_ST_HITCAP: the host decides */
}

// results of the searches that were run again with longer hit lists (nabwa_batch_sync): the q-th search of the list -> its read; its
// rows are block + q * cap3, entered in the table of grown row blocks at slot0 + q, which the read's wide_idx names from now on
__global__ __launch_bounds__(256) void scatter_grown_kernel(int n2, const int32_t *__restrict__ ids, const int32_t *__restrict__ n_aln3,
															const int32_t *__restrict__ max_ent3, const uint8_t *__restrict__ status3,
															int32_t *__restrict__ n_aln, int32_t *__restrict__ max_ent, uint8_t *__restrict__ status,
															int32_t *__restrict__ wide_idx, const uint4 *block, size_t cap3, const uint4 **__restrict__ grown, int slot0)
{
	const int q = blockIdx.x * 256 + threadIdx.x;
	if (q >= n2) return;
	const int rid = ids[q];
	max_ent[rid] = max_ent3[q];
	if (status3[q] == NABWA_ST_OK) { n_aln[rid] = n_aln3[q]; status[rid] = NABWA_ST_GROWN; wide_idx[rid] = slot0 + q; grown[slot0 + q] = block + (size_t)q * cap3; }
	else { n_aln[rid] = 0; status[rid] = status3[q]; }
}
extern "C" void nabwa_launch_scatter_grown(int n2, const int32_t *ids, const int32_t *n_aln3, const int32_t *max_ent3, const uint8_t *status3,
										   int32_t *n_aln, int32_t *max_ent, uint8_t *status, int32_t *wide_idx, const uint4 *block, size_t cap3,
										   const uint4 **grown, int slot0, hipStream_t s)
{
	if (n2 <= 0) return;
	hipLaunchKernelGGL(scatter_grown_kernel, dim3((n2 + 255) / 256), dim3(256), 0, s, n2, ids, n_aln3, max_ent3, status3, n_aln, max_ent, status, wide_idx, block, cap3, grown, slot0);
}

// the reads that go to the wide passes get a row each in the wide result arrays; it stays theirs over the tiers
__global__ __launch_bounds__(256) void assign_slots_kernel(int n2, const int32_t *__restrict__ ids, int32_t *__restrict__ wide_idx)
{
	const int j = blockIdx.x * 256 + threadIdx.x;
	if (j < n2) wide_idx[ids[j]] = j;
}

extern "C" void nabwa_launch_assign_slots(int n2, const int32_t *ids, int32_t *wide_idx, hipStream_t s)
{
	if (n2 <= 0) return;
	hipLaunchKernelGGL(assign_slots_kernel, dim3((n2 + 255) / 256), dim3(256), 0, s, n2, ids, wide_idx);
}

extern "C" void nabwa_launch_scatter_wide(int n2, const int32_t *ids, const int32_t *n_aln2, const int32_t *max_ent2,
										  const uint8_t *status2, int32_t *n_aln, int32_t *max_ent, uint8_t *status,
										  int32_t *wide_idx, hipStream_t s)
{
	if (n2 <= 0) return;
	hipLaunchKernelGGL(scatter_wide_kernel, dim3((n2 + 255) / 256), dim3(256), 0, s, n2, ids, n_aln2, max_ent2, status2,
					   n_aln, max_ent, status, wide_idx);
}

__device__ __forceinline__ const uint4 *rows_of(int i, const uint4 *aln, int aln_cap, const uint8_t *status,
												const int32_t *wide_idx, const uint4 *aln2, int aln_cap2, const uint4 *const *grown)
{
	const int st = status[i];
	if (st == NABWA_ST_GROWN) return grown[wide_idx[i]];           /* a hit list that outgrew the wide rows: its own block (nabwa_batch_sync) */
	return st == NABWA_ST_WIDE ? aln2 + (size_t)wide_idx[i] * aln_cap2 : aln + (size_t)i * aln_cap;
}

// compaction: rows of read i go to out[row_off[i] ...].  map: null, or the read whose rows read i takes (NABWA_DEDUP: n and row_off are the
// caller's, n_aln and the rows those of the reads searched); a negative map value -1 - k: the rows of the cache entry at arena + 16 * cent[k]
// (NABWA_DEDUP_CACHE, dedup_cache_body.hpp)
__global__ __launch_bounds__(256) void gather_kernel(int n, const int32_t *__restrict__ map, const uint32_t *__restrict__ cent, const uint8_t *__restrict__ arena,
												 const int32_t *__restrict__ n_aln, const uint32_t *__restrict__ row_off,
												 const uint4 *__restrict__ aln, int aln_cap, const uint8_t *__restrict__ status,
												 const int32_t *__restrict__ wide_idx, const uint4 *__restrict__ aln2, int aln_cap2,
												 const uint4 *const *__restrict__ grown, uint4 *__restrict__ out)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const int rd = map ? map[i] : i;
	const uint8_t *e = rd < 0 ? arena + (size_t)cent[-1 - rd] * 16 : 0;
	const int na = e ? dcache_n_aln(e) : n_aln[rd];
	const uint4 *src = e ? dcache_rows(e) : rows_of(rd, aln, aln_cap, status, wide_idx, aln2, aln_cap2, grown);
	uint4 *dst = out + row_off[i];
	for (int j = 0; j < na; ++j) dst[j] = src[j];
}

extern "C" void nabwa_launch_gather(int n, const int32_t *map, const uint32_t *cent, const uint8_t *arena, const int32_t *n_aln, const uint32_t *row_off, const uint4 *aln, int aln_cap,
									const uint8_t *status, const int32_t *wide_idx, const uint4 *aln2, int aln_cap2,
									const uint4 *const *grown, uint4 *out, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(gather_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, map, cent, arena, n_aln, row_off, aln, aln_cap, status,
					   wide_idx, aln2, aln_cap2, grown, out);
}

// order-independent checksum over all hits: sum of a mix of (read, row index, row words)
__device__ __forceinline__ uint64_t mix64(uint64_t x)
{
	x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33;
	return x;
}

// (map, cent and arena as in gather_kernel: read i, the caller's, is summed with the rows of read map[i] or of its cache entry)
__global__ __launch_bounds__(256) void checksum_kernel(int n, const int32_t *__restrict__ map, const uint32_t *__restrict__ cent, const uint8_t *__restrict__ arena,
												   const int32_t *__restrict__ n_aln, const uint4 *__restrict__ aln,
												   int aln_cap, const uint8_t *__restrict__ status, const int32_t *__restrict__ wide_idx,
												   const uint4 *__restrict__ aln2, int aln_cap2, const uint4 *const *__restrict__ grown,
												   unsigned long long *__restrict__ sum, unsigned long long *__restrict__ rows)
{
	const int i = blockIdx.x * 256 + threadIdx.x;
	uint64_t s = 0, r = 0;
	if (i < n) {
		const int rd = map ? map[i] : i;
		const uint8_t *e = rd < 0 ? arena + (size_t)cent[-1 - rd] * 16 : 0;
		const int na = e ? dcache_n_aln(e) : n_aln[rd];
		const uint4 *src = e ? dcache_rows(e) : rows_of(rd, aln, aln_cap, status, wide_idx, aln2, aln_cap2, grown);
		r = (uint64_t)na;
		s = mix64(((uint64_t)i << 20) ^ (uint64_t)na ^ 0x9e3779b97f4a7c15ULL);
		for (int j = 0; j < na; ++j) {
			const uint4 h = src[j];
			s += mix64(((uint64_t)i << 32 | (uint32_t)j) ^ mix64((uint64_t)h.x << 32 | h.y) ^ mix64((uint64_t)h.z << 32 | h.w) * 3ULL);
		}
	}
	for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o); r += __shfl_down(r, o); }
	if ((threadIdx.x & 63) == 0) { atomicAdd(sum, (unsigned long long)s); atomicAdd(rows, (unsigned long long)r); }
}

extern "C" void nabwa_launch_checksum(int n, const int32_t *map, const uint32_t *cent, const uint8_t *arena, const int32_t *n_aln, const uint4 *aln, int aln_cap, const uint8_t *status,
									  const int32_t *wide_idx, const uint4 *aln2, int aln_cap2,
									  const uint4 *const *grown, unsigned long long *sum, unsigned long long *rows, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(checksum_kernel, dim3((n + 255) / 256), dim3(256), 0, s, n, map, cent, arena, n_aln, aln, aln_cap, status, wide_idx,
					   aln2, aln_cap2, grown, sum, rows);
}

// Work order of the search kernel by kernel W's class of a read = the smaller of its two strands' restart counts, i.e. a
// lower bound of the differences of its best hit: 0 (an exact occurrence exists), 1, 2+.  A search can take 10^4 dependent
// trips (tens of ms; the launch cannot end before its longest search does), so the long searches must START first:
// order 2+, 1, 0.  Class 0 reads run alike and close the launch in lockstep waves (64 reads at a time); the others go lane
// by lane.  (Tried: class 1 in lockstep waves -- its reads differ too much; a finer order 4+, 3, 2, 1, 0 -- the few hundred
// longest searches then sit in ONE wave's first block and run one after the other; those reads one per wave, or their waves
// at raised issue priority -- a trip is no shorter for it.  Mixed into the 2+ class they start in ~650 different waves at once.)
// cnt: the class counter block (search_slots.hpp, NCLS_*): pass 1 fills the class sizes, pass 2 moves the cursors and sets the
// first work item of class 0 (*n_sync of the search kernel).  One wave handles 1024 consecutive reads with one atomic per class.
template <int PASS>
__global__ __launch_bounds__(256) void partition_kernel(int n, const uint8_t *__restrict__ cls, int32_t *__restrict__ ids, unsigned int *__restrict__ cnt)
{
	const unsigned int lane = threadIdx.x & 63u;
	const long wave = ((long)blockIdx.x * 256 + threadIdx.x) >> 6;
	const long first = wave * 1024;
	if (PASS == 2 && blockIdx.x == 0 && threadIdx.x == 0) { unsigned int x = 0; for (int q = 1; q < NCLS_N; ++q) x += cnt[NCLS_SIZE + q]; cnt[NCLS_FIRST0] = x; }
	if (first >= n) return;
	unsigned int num[NCLS_N]; int cl[16];
#pragma unroll
	for (int q = 0; q < NCLS_N; ++q) num[q] = 0;
#pragma unroll
	for (int g = 0; g < 16; ++g) {
		const long i = first + g * 64 + lane;
		const uint8_t c0 = i < n ? cls[2 * i] : 0, c1 = i < n ? cls[2 * i + 1] : 0;
		cl[g] = i < n ? (int)(c0 < c1 ? c0 : c1) : -1;
		if (cl[g] > NCLS_N - 1) cl[g] = NCLS_N - 1;
#pragma unroll
		for (int q = 0; q < NCLS_N; ++q) num[q] += (unsigned int)__popcll(__ballot(cl[g] == q));
	}
	if (PASS == 1) {
		if (lane == 0) for (int q = 0; q < NCLS_N; ++q) if (num[q]) atomicAdd(cnt + NCLS_SIZE + q, num[q]);
		return;
	}
	unsigned int base[NCLS_N];
#pragma unroll
	for (int q = 0; q < NCLS_N; ++q) base[q] = 0;
	if (lane == 0) {
		unsigned int start = 0;
		for (int q = NCLS_N - 1; q >= 0; --q) { if (num[q]) base[q] = start + atomicAdd(cnt + NCLS_CURSOR + q, num[q]); start += cnt[NCLS_SIZE + q]; }
	}
#pragma unroll
	for (int q = 0; q < NCLS_N; ++q) base[q] = __shfl(base[q], 0);
#pragma unroll
	for (int g = 0; g < 16; ++g) {
		const long i = first + g * 64 + lane;
		const unsigned long long below = (1ull << lane) - 1ull;
#pragma unroll
		for (int q = 0; q < NCLS_N; ++q) {
			const unsigned long long mq = __ballot(cl[g] == q);
			if (cl[g] == q) ids[base[q] + (unsigned int)__popcll(mq & below)] = (int32_t)i;
			base[q] += (unsigned int)__popcll(mq);
		}
	}
}

extern "C" void nabwa_launch_partition(int n, const uint8_t *cls, int32_t *ids, unsigned int *cnt, hipStream_t s)
{
	if (n <= 0) return;
	hipLaunchKernelGGL(partition_kernel<1>, dim3((n + 4095) / 4096), dim3(256), 0, s, n, cls, ids, cnt);
	hipLaunchKernelGGL(partition_kernel<2>, dim3((n + 4095) / 4096), dim3(256), 0, s, n, cls, ids, cnt);
}
