// nabwa_internal.hpp -- host-side structures shared by the translation units of libnabwa.so
#pragma once
#include <stdint.h>
#include <stdio.h>
#include <mutex>
#include <string>
#include <vector>
#include "../../include/nabwa.h"
#include "fm_search.hpp"
#include "host_util.hpp"

struct nabwa_ann { int64_t offset; int32_t len, n_ambs; std::string name; };    // bntann1_t, bntseq.h:39-45
struct nabwa_hole { int64_t offset; int32_t len; char amb; };                   // bntamb1_t, bntseq.h:47-51

struct nabwa_reference {          // bntseq_t + the packed reference (bntseq.h:53-61, bwtio.c pac)
	int64_t l_pac; uint32_t seed;
	std::vector<nabwa_ann> anns;
	std::vector<nabwa_hole> holes;
	std::vector<uint8_t> pac;     // 2 bits per base, 4 bases per byte, first base in the top bits (bwtaln.h:33)
};

/* The cross-batch read cache of NABWA_DEDUP_CACHE (layout and protocol: dedup_cache_body.hpp).  One per index, made by the first batch
 * that asks for it, out of the index's pool, freed with the index.  mu covers every lookup stage and every insert stage of the batches on this
 * index including the drain of their stream, so no lookup kernel runs beside an insert kernel; it also guards everything below. */
struct nabwa_dedup_cache {
	std::mutex mu;
	unsigned long long *d_slots = nullptr; uint32_t n_slots = 0;     /* the table */
	uint8_t *d_arena = nullptr; uint64_t arena_bytes = 0;             /* the entries, append-only */
	unsigned long long *d_ctr = nullptr;                              /* DC_* counters */
	uint64_t reserved = 0;                                            /* device bytes of the three */
	bool has_sig = false; uint64_t sig = 0;                           /* the option signature the entries were made under */
	int pins = 0;                                                     /* live batches that hold references into the arena */
	uint64_t used = 0, entries = 0;                                   /* as of the last insert stage */
	uint64_t lookups = 0, served = 0, flushes = 0, bypasses = 0;
};

struct nabwa_index {
	int device = 0;
	DevBwt bwt[2] = {};
	uint4 *bk[2] = {};
	uint32_t *sa[2] = {};
	uint32_t *sa_full[2] = {}, *isa[2] = {}, *text[2] = {};   // text-mode companions (nabwa_dev.hpp), null when switched off
	uint2 *kmer[2] = {}, *kmer_top[2] = {};  // interval table: levels 1..LW back to back; level T on its own when T > LW (else inside the former)
	uint64_t bytes = 0;
	int kmer_T_pick = -1;           // depth of the interval tables, decided when the first direction is built
	uint32_t kmer_pk[2][NABWA_PK_LEVELS] = {};   // per level 0..16 its primary key (fm_index.hip), ~0u where it has none; behind the ixtab words of every batch
	nabwa_reference *ref = nullptr;
	nabwa_reference *ref_nt = nullptr;   // colour index: the annotations of `ref` over the bases of <prefix>.nt.pac (cs2nt.hip)
	uint8_t *d_ntpac = nullptr;          // ... and those bases in HBM, with their size in bytes
	uint64_t ntpac_bytes = 0;
	struct nabwa_dev_pool *pool = nullptr;   // released working buffers of earlier batches, kept for the next one (dev_pool.hpp)
	/* the finishing chains' device path (finish_gpu.hip): the bases of `ref` and the hole tables of `ref` / `ref_nt` in HBM, uploaded by the
	 * first call that needs them -- the chains run on several threads, hence the lock -- and counted in `bytes` */
	std::mutex fin_mu;
	uint8_t *d_pac = nullptr; uint64_t pac_bytes = 0;
	void *d_holes[2] = {}; uint64_t holes_bytes[2] = {}; int n_holes_dev[2] = {};
	bool fin_ready[2] = {};
	std::mutex dcache_mu;                      /* guards the pointer below while the first batches make the cache */
	nabwa_dedup_cache *dcache = nullptr;
};

/* nabwa_index.hip: the index's read cache of at most `mib` MiB, made on first use (NABWA_EINVAL when that is more than the device has free; a
 * later call returns the cache there is, whatever its size); emptied -- the caller holds c->mu and the cache has no pins */
int nabwa_dcache_get(nabwa_index *ix, long mib, nabwa_dedup_cache **out);
int nabwa_dcache_reset(nabwa_index *ix, nabwa_dedup_cache *c);

/* a failed HIP call: "<expr> failed: <hip error> (<file>:<line>)" as the last error, NABWA_ENODEV as the result */
static inline int nabwa_hip_fail(hipError_t e, const char *expr, const char *file, int line)
{
	char b[512]; snprintf(b, sizeof b, "%s failed: %s (%s:%d)", expr, hipGetErrorString(e), file, line);
	return nabwa_fail(NABWA_ENODEV, "%s", b);
}
#define HIP_CHECK(x) do { const hipError_t e_ = (x); if (e_ != hipSuccess) return nabwa_hip_fail(e_, #x, __FILE__, __LINE__); } while (0)

/* entry points on records of any stride whose head is a nabwa_se_t (nabwa_pe_t starts with one), for the files that work in place
 * (se_finish.hip) */
int nabwa_se_posn_strided(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
						  const int32_t *n_aln, const nabwa_aln1_t *aln, const uint8_t *n_occ_v, uint64_t *rng48, void *out_base, size_t stride);
int nabwa_se_refine_strided(nabwa_index_t *ix, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, void *out_base, size_t stride);
/* <prefix>.ann, .amb and .pac into a new nabwa_reference (se_finish.hip) */
int nabwa_reference_read(const char *prefix, nabwa_reference **out);
/* colour space (cs2nt.hip): bwa_cs2nt_core for every mapped record on the GPU -- the decoded reads go to nt_seq (the read reversed, as
 * bwa_seq_t.seq is held here), nt_rseq (its reverse complement) and nt_qual (qualities + 33, read order) from off[i] on, and len =
 * full_len = the decoded length in the records.  times (may be null): [0] += seconds of this stage, [1] += milliseconds of its kernels */
int nabwa_cs2nt_records(nabwa_index_t *ix, void *base, size_t stride, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq,
						const uint8_t *qual, uint8_t *nt_seq, uint8_t *nt_rseq, uint8_t *nt_qual, double *times);
/* the wide rows of a batch's pairs into finish_pair's position cache, in record order (pe_finish.hip) */
void nabwa_poscache_register(nabwa_poscache_t *cache, int max_occ, int n, const int *first, const int32_t *n_aln, const int64_t *row0,
							 const nabwa_aln1_t *rows, const nabwa_pe_t *res);

