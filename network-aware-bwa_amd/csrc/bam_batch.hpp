// bam_batch.hpp -- a batch of BAM records on its way through bam2bam's two passes: what nabwa_bam_batch_create makes (bam_front.cpp) and the
// passes work on (bam_batch.hip).  The index is only named here, so the front-end and its CPU tests see the batch without any HIP header.
#pragma once
#include <stdint.h>
#include <new>
#include <string>
#include <vector>
#include "../../include/nabwa.h"
#include "bam_rec.hpp"
#include "host_pool.hpp"
#include "host_util.hpp"

struct nabwa_index;

static const size_t BAM_MIN_N = 8192;          /* records below which the host work of a batch stays on one thread */

/* The parsed records of a batch: pooled memory like the other per-batch blocks, constructed and destroyed by all threads (a std::vector of
 * a million records does both on one thread, zero fill and page faults included: 15 ms of a 60 ms create). */
struct RecArr {
	Pooled<BamRec> blk; size_t n;
	RecArr() : n(0) {}
	~RecArr() { clear(); }
	bool make(size_t m)
	{
		clear();
		if (!blk.take(sizeof(BamRec) * (m ? m : 1))) return false;
		n = m;
		BamRec *const q = blk.get();
		host_parallel(host_threads(m, BAM_MIN_N), m, [q](int, size_t lo, size_t hi) { for (size_t i = lo; i < hi; ++i) new (q + i) BamRec(); });
		return true;
	}
	void clear()
	{
		if (blk) {
			BamRec *const q = blk.get();
			host_parallel(host_threads(n, BAM_MIN_N), n, [q](int, size_t lo, size_t hi) { for (size_t i = lo; i < hi; ++i) q[i].~BamRec(); });
			blk.give();
		}
		n = 0;
	}
	size_t size() const { return n; }
	bool empty() const { return n == 0; }
	BamRec &operator[](size_t i) { return blk[i]; }
	const BamRec &operator[](size_t i) const { return blk[i]; }
	void swap(RecArr &o) { blk.swap(o.blk); const size_t m = n; n = o.n; o.n = m; }
};

/* hit rows as they come back from the device: no zero fill on one thread in front of the copy (a std::vector's resize), pooled like the rest.
 * Growing it loses what it held (every caller fills it whole afterwards); shrinking keeps it. */
struct RowArr {
	RawBytes raw; size_t n;
	RowArr() : n(0) {}
	bool resize(size_t m) { if (m * sizeof(nabwa_aln1_t) > raw.cap) { if (!raw.alloc(m * sizeof(nabwa_aln1_t))) { n = 0; return false; } } n = m; return true; }
	size_t size() const { return n; }
	nabwa_aln1_t *data() { return (nabwa_aln1_t*)raw.p; }
	const nabwa_aln1_t *data() const { return (const nabwa_aln1_t*)raw.p; }
};

struct nabwa_bam_batch {
	nabwa_index *ix; nabwa_gap_opt_t opt; nabwa_pe_opt_t popt;
	Pooled<uint8_t> arena;                         /* where the records' bytes live; declared before rec: it outlives the records */
	RecArr rec;                                    /* in logical-record order: singletons, and pairs as read 1, read 2 */
	std::vector<int> kind;                         /* per logical record: 1 or 2 */
	std::vector<int> first;                        /* per logical record: index of its first read */
	std::vector<int> rg;                           /* per logical record: its read group, an index into rg_names */
	std::vector<std::string> rg_names;
	std::vector<uint8_t> skip;                     /* per logical record: a flagged duplicate that passes through untouched (--skip-duplicates; unique(), bam2bam.c:595-606) */
	uint32_t flags;                                /* NABWA_BAM_* */
	std::vector<int64_t> off; RawBytes seq, rseq; std::vector<int32_t> full_len;     /* the encoded reads, one per BAM record */
	std::vector<int32_t> n_aln, max_ent; RowArr rows; std::vector<int64_t> row0;
	Pooled<nabwa_pe_t> res;                        /* per read: the chain's record (singletons use .se only); raw memory: only what a phase fills is valid */
	int phase;                                     /* 0 created, 1 positioned, 2 finished */
	bool searched;                                 /* nabwa_bam_batch_search ran */
	std::vector<uint8_t> parked; std::vector<uint64_t> parked_at;     /* what pass 1 left in res, packed, while a batch with pairs waits for pass 2 */
	std::vector<uint8_t> wire_multi;                /* nabwa_bam_batch_positioned: the other hits of the reads as raw bwt_multi1_t */
	nabwa_bam_batch() : ix(0), flags(0), phase(0), searched(false) {}
	~nabwa_bam_batch() { res.give(); rec.clear(); arena.give(); }      /* in this order the blocks go back to the pool, ahead of the members' own turn */
};
