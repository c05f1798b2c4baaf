// dedup_cache_body.hpp -- the bodies of the cross-batch read cache (NABWA_DEDUP_CACHE; kernels in dedup_cache_kernels.hip, the
// host side in nabwa_batch.hip and nabwa_index.hip): how an entry lies in the arena, how the table is probed, the exact comparison of a read
// with an entry, and the claim / reserve / write steps of an insert.
//
//   table   n_slots (a power of two) 64-bit slots.  0: empty.  DCACHE_CLAIMED: claimed by an insert that then found the arena full; never
//           matches, never freed.  Else: the top 24 bits of the entry's hash << 40 | (the entry's arena offset / 16 + 1).
//   probe   slot (hash & mask) + p, p = 0 .. DCACHE_PROBES - 1, modulo n_slots (mask: NABWA_DEDUP_HASH_BITS, all ones by default).  A lookup
//           ends at the first empty slot, an insert takes it; after DCACHE_PROBES slots both give up: the read is searched / not inserted.
//   entry   16-byte aligned, never moved: DcacheHdr (32 bytes), seq and rseq each padded with zero bytes to whole 16-byte chunks, then
//           n_aln rows of 16 bytes.  dcache_entry_size() bytes in all.
//
// A lookup never trusts the hash: an entry answers for a read only when hash, length, max_diff, max_gapo and every byte of both strands agree.
// An entry's body is written by the launch that claimed its slot and is read by later launches only (the host never runs a lookup beside an
// insert); within a launch only the slot claim (compare-and-swap) and the arena's bump counter (add) are contended, both device-scope atomics.
// Every loop is bounded by DCACHE_PROBES, the read's length or its row count.  No arrays beyond a header: no scratch.
// Compiled for gfx950 and, with NABWA_EMU (tests/emu/dedup_cache_emu.cpp, test infrastructure), by g++.
#pragma once
#include "dedup_body.hpp"

#define DCACHE_PROBES  16                  /* slots a lookup or an insert looks at, at most */
#define DCACHE_HDR     32u
#define DCACHE_CLAIMED 0xffffffffffffffffULL
/* the cache's counter block (unsigned long long each) */
enum { DC_BUMP = 0,      /* arena bytes handed out or asked for: may pass the arena's size once it is full */
       DC_USED,          /* bytes of the entries written */
       DC_ENTRIES,
       DC_FULL,          /* reads not inserted: no slot within the probe bound, or no room in the arena */
       DC_SKIPPED,       /* reads not inserted: more rows than the cap, or a search that did not complete */
       DC_WORDS = 8 };

#ifdef NABWA_EMU
static inline unsigned long long dcache_cas(unsigned long long *p, unsigned long long expect, unsigned long long v) { const unsigned long long o = *p; if (o == expect) *p = v; return o; }
static inline unsigned long long dcache_add(unsigned long long *p, unsigned long long v) { const unsigned long long o = *p; *p = o + v; return o; }
static inline unsigned long long dcache_load(const unsigned long long *p) { return *p; }
static inline void dcache_store(unsigned long long *p, unsigned long long v) { *p = v; }
#else
__device__ __forceinline__ unsigned long long dcache_cas(unsigned long long *p, unsigned long long expect, unsigned long long v) { return atomicCAS(p, expect, v); }
__device__ __forceinline__ unsigned long long dcache_add(unsigned long long *p, unsigned long long v) { return atomicAdd(p, v); }
__device__ __forceinline__ unsigned long long dcache_load(const unsigned long long *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void dcache_store(unsigned long long *p, unsigned long long v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#endif

struct DcacheHdr {
	uint64_t hash;                 /* dedup_hash_finish over the read: all 64 bits, whatever the probe mask */
	uint32_t len;
	uint8_t md, mg; uint16_t zero; /* the max_diff and max_gapo the read was searched with */
	int32_t n_aln, max_ent;
	uint32_t rows_off, size;       /* from the entry's start, bytes */
};

DEDUP_FN uint32_t dcache_padded(int L) { return ((uint32_t)L + 15u) & ~15u; }
DEDUP_FN uint32_t dcache_entry_size(int L, int n_aln) { return DCACHE_HDR + 2u * dcache_padded(L) + 16u * (uint32_t)n_aln; }
DEDUP_FN uint64_t dcache_slot_index(uint64_t hash, uint64_t mask, uint32_t n_slots, int p) { return ((hash & mask) + (uint64_t)p) & (uint64_t)(n_slots - 1u); }
DEDUP_FN unsigned long long dcache_slot_value(uint64_t hash, uint64_t off16) { return (hash >> 40) << 40 | (off16 + 1u); }

/* lookup: from probe *p on, the next slot that may hold the read -> its entry's arena offset / 16 + 1, *p behind it; 0 when the chain ends
 * (an empty slot) or the probe bound is reached */
DEDUP_FN uint64_t dcache_next_candidate(const unsigned long long *slots, uint32_t n_slots, uint64_t hash, uint64_t mask, int *p)
{
	while (*p < DCACHE_PROBES) {
		const unsigned long long v = slots[dcache_slot_index(hash, mask, n_slots, *p)];
		++*p;
		if (v == 0) { *p = DCACHE_PROBES; return 0; }
		if (v != DCACHE_CLAIMED && (v >> 40) == (hash >> 40)) return v & 0xffffffffffULL;
	}
	return 0;
}

/* lookup: is entry e the read of length L at seq + o / rseq + o, searched with md and mg?  Lane t's chunks; every lane reads the header */
DEDUP_FN bool dcache_match_part(const uint8_t *e, uint64_t hash, const uint8_t *seq, const uint8_t *rseq, int64_t o, int L, int md, int mg, int t)
{
	DcacheHdr h;
	__builtin_memcpy(&h, e, sizeof h);
	if (h.hash != hash || h.len != (uint32_t)L || h.md != md || h.mg != mg) return false;
	const uint32_t pl = dcache_padded(L);
	bool same = true;
	const int NC = (L + 15) >> 4;
	for (int c = t; c < NC; c += DEDUP_LANES) {
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			uint64_t a[2], b[2];
			dedup_load_chunk((st ? rseq : seq) + o + 16 * (int64_t)c, L - 16 * c, a);
			__builtin_memcpy(b, e + DCACHE_HDR + (st ? pl : 0u) + 16u * (uint32_t)c, 16);      /* an entry's chunks are whole: zero bytes behind the read */
			same = same && a[0] == b[0] && a[1] == b[1];
		}
	}
	return same;
}

/* insert, one lane per read: the first empty slot of the read's chain is claimed -> its index, or -1 within the probe bound there is none */
DEDUP_FN int64_t dcache_claim_slot(unsigned long long *slots, uint32_t n_slots, uint64_t hash, uint64_t mask)
{
	for (int p = 0; p < DCACHE_PROBES; ++p) {
		const uint64_t idx = dcache_slot_index(hash, mask, n_slots, p);
		if (dcache_cas(slots + idx, 0ull, DCACHE_CLAIMED) == 0ull) return (int64_t)idx;
	}
	return -1;
}

/* insert, one lane per read: `size` bytes of the arena -> their offset, or -1 when they do not fit */
DEDUP_FN int64_t dcache_reserve(unsigned long long *ctr, uint64_t arena_bytes, uint32_t size)
{
	if (dcache_load(ctr + DC_BUMP) + size > arena_bytes) return -1;      /* full: leave the counter alone */
	const unsigned long long o = dcache_add(ctr + DC_BUMP, (unsigned long long)size);
	return o + size <= arena_bytes ? (int64_t)o : -1;
}

/* insert, one lane per read: the whole decision.  eligible: the search is complete and its rows are within the cap.  -> the entry's arena
 * offset (a multiple of 16) with its slot in *slot, or -1; the counters say which.  A slot whose reserve then fails stays DCACHE_CLAIMED. */
DEDUP_FN long long dcache_insert_claim(unsigned long long *slots, uint32_t n_slots, uint64_t hash, uint64_t mask, unsigned long long *ctr, uint64_t arena_bytes,
									   int L, int n_aln, bool eligible, int64_t *slot)
{
	*slot = -1;
	if (!eligible) { dcache_add(ctr + DC_SKIPPED, 1ull); return -1; }
	const uint32_t size = dcache_entry_size(L, n_aln);
	long long where = -1;
	if (dcache_load(ctr + DC_BUMP) + size <= arena_bytes) *slot = dcache_claim_slot(slots, n_slots, hash, mask);      /* (a full arena costs no slot) */
	if (*slot >= 0) where = dcache_reserve(ctr, arena_bytes, size);
	if (where < 0) dcache_add(ctr + DC_FULL, 1ull);
	else { dcache_add(ctr + DC_USED, (unsigned long long)size); dcache_add(ctr + DC_ENTRIES, 1ull); }
	return where;
}

/* insert: lane t's share of the entry at e -- lane 0 the header, chunk c of both strands by lane c % 16 (zero bytes behind the read), row j
 * by lane j % 16.  seq + o / rseq + o: the read; nothing at or beyond its L bytes is touched */
DEDUP_FN void dcache_write_part(uint8_t *e, uint64_t hash, const uint8_t *seq, const uint8_t *rseq, int64_t o, int L, int md, int mg,
								int n_aln, int max_ent, const uint4 *rows, int t)
{
	const uint32_t pl = dcache_padded(L);
	if (t == 0) {
		DcacheHdr h;
		h.hash = hash; h.len = (uint32_t)L; h.md = (uint8_t)md; h.mg = (uint8_t)mg; h.zero = 0; h.n_aln = n_aln; h.max_ent = max_ent;
		h.rows_off = DCACHE_HDR + 2u * pl; h.size = dcache_entry_size(L, n_aln);
		__builtin_memcpy(e, &h, sizeof h);
	}
	const int NC = (L + 15) >> 4;
	for (int c = t; c < NC; c += DEDUP_LANES) {
#pragma unroll
		for (int st = 0; st < 2; ++st) {
			uint64_t w[2];
			dedup_load_chunk((st ? rseq : seq) + o + 16 * (int64_t)c, L - 16 * c, w);
			__builtin_memcpy(e + DCACHE_HDR + (st ? pl : 0u) + 16u * (uint32_t)c, w, 16);
		}
	}
	uint4 *dst = (uint4*)(e + DCACHE_HDR + 2u * pl);
	for (int j = t; j < n_aln; j += DEDUP_LANES) dst[j] = rows[j];
}

/* what the batch's read-back takes from an entry (batch_kernels.hip, dedup_kernels.hip) */
DEDUP_FN int dcache_n_aln(const uint8_t *e) { DcacheHdr h; __builtin_memcpy(&h, e, sizeof h); return h.n_aln; }
DEDUP_FN int dcache_max_ent(const uint8_t *e) { DcacheHdr h; __builtin_memcpy(&h, e, sizeof h); return h.max_ent; }
DEDUP_FN const uint4 *dcache_rows(const uint8_t *e) { DcacheHdr h; __builtin_memcpy(&h, e, sizeof h); return (const uint4*)(e + h.rows_off); }
