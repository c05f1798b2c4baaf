// launchers.hpp -- the host-callable launchers and occupancy queries of fm_index.hip, fm_search.hip, batch_kernels.hip, fm_deep.hip, dedup_kernels.hip, dedup_cache_kernels.hip, bgzf_deflate.hip, bgzf_inflate.hip, finish_kernels.hip, damage_kernels.hip, markdup_kernels.hip and bai_kernels.hip, declared once.
// The defining files and every host unit that calls one include this header, so a parameter list that differs between the two sides
// is a compile error (C linkage carries no types).  Host side only: the kernel headers (nabwa_dev.hpp, fm_search.hpp, fm_deep.hpp,
// fm_deep_body.hpp) do not include it -- the CPU emulation of the tests compiles those without HIP.
#pragma once
#include <hip/hip_runtime.h>
#include "fm_deep.hpp"

extern "C" {
/* fm_index.hip */
void nabwa_launch_repack(const uint32_t *w, uint32_t seq_len, uint32_t n_buckets, uint4 *out, hipStream_t s);
void nabwa_launch_kmer_level(const DevBwt *B, const uint2 *prev, uint2 *cur, uint64_t n_cur, hipStream_t s);
void nabwa_launch_kmer_primary(const uint2 *lv, uint64_t n_keys, uint32_t primary, uint32_t *out, hipStream_t s);
void nabwa_launch_sa_fill(const DevBwt *B, uint32_t *sa_full, uint32_t *isa, uint8_t *text_bytes, hipStream_t s);
void nabwa_launch_text_pack(const uint8_t *bytes, uint32_t n, uint32_t n_words, uint32_t *out, hipStream_t s);
void nabwa_launch_sa_lookup(const DevBwt *B, int n, const uint8_t *which, const uint32_t *k, uint32_t *out, hipStream_t s);
void nabwa_launch_occ4(const DevBwt *B, int n, const uint32_t *k, uint32_t *out, hipStream_t s);
/* fm_search.hip */
void nabwa_launch_fm_search(const SearchParams *P, int n_blocks, hipStream_t s);
void nabwa_launch_fm_width(const SearchParams *P, int n_blocks, hipStream_t s);
int nabwa_width_occupancy(int text_mode);      /* of kernel W's instantiation for these forms (fm_search.hpp: TM_W_*) */
int nabwa_search_occupancy(int ns);
/* batch_kernels.hip */
/* map (checksum, gather): null, or for each of the n reads the read whose results it takes (NABWA_DEDUP: the caller's read -> the read searched);
 * a map value -1 - k: served read k of NABWA_DEDUP_CACHE, whose entry (dedup_cache_body.hpp) lies at arena + 16 * cent[k] */
void nabwa_launch_checksum(int n, const int32_t *map, const uint32_t *cent, const uint8_t *arena, const int32_t *n_aln, const uint4 *aln, int aln_cap, const uint8_t *status,
						   const int32_t *wide_idx, const uint4 *aln2, int aln_cap2, const uint4 *const *grown,
						   unsigned long long *sum, unsigned long long *rows, hipStream_t s);
void nabwa_launch_collect(int n, const uint8_t *status, int32_t *ids, unsigned int *count, int which, hipStream_t s);
void nabwa_launch_collect_keyed(int n, const uint8_t *status, int32_t *ids, unsigned int *count, int which,
								const uint8_t *cls, const uint8_t *md, int max_key, const int32_t *n_aln, int aln_cap, hipStream_t s);
void nabwa_launch_assign_slots(int n2, const int32_t *ids, int32_t *wide_idx, hipStream_t s);
void nabwa_launch_scatter_grown(int n2, const int32_t *ids, const int32_t *n_aln3, const int32_t *max_ent3, const uint8_t *status3,
								 int32_t *n_aln, int32_t *max_ent, uint8_t *status, int32_t *wide_idx, const uint4 *block, size_t cap3,
								 const uint4 **grown, int slot0, hipStream_t s);
void nabwa_launch_scatter_wide(int n2, const int32_t *ids, const int32_t *n_aln2, const int32_t *max_ent2,
							   const uint8_t *status2, int32_t *n_aln, int32_t *max_ent, uint8_t *status,
							   int32_t *wide_idx, hipStream_t s);
void nabwa_launch_gather(int n, const int32_t *map, const uint32_t *cent, const uint8_t *arena, const int32_t *n_aln, const uint32_t *row_off, const uint4 *aln, int aln_cap,
						 const uint8_t *status, const int32_t *wide_idx, const uint4 *aln2, int aln_cap2,
						 const uint4 *const *grown, uint4 *out, hipStream_t s);
void nabwa_launch_partition(int n, const uint8_t *cls, int32_t *ids, unsigned int *cnt, hipStream_t s);
void nabwa_launch_padded_len(int n, const int64_t *off, int64_t *plen, hipStream_t s);
void nabwa_launch_pad_reads(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const int64_t *poff,
							uint8_t *pseq, uint8_t *prseq, int32_t *rd_len, uint32_t *rd_key, int T, int seed_len, uint32_t *rd_pack, int pack_stride,
							const uint8_t *md_tab, const uint8_t *mg_tab, uint8_t *rd_md, uint8_t *rd_mg, hipStream_t s);
/* dedup_kernels.hip (dedup_body.hpp): the duplicate-read stage of a batch, in the order nabwa_batch.hip runs it.  16 lanes per read in hash, verify
 * and compact; no kernel reads seq / rseq at or beyond off[n] or writes the compact buffers at or beyond coff[n_u] */
void nabwa_launch_dedup_hash(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, uint64_t mask, uint64_t *keys, uint32_t *ids, hipStream_t s);
void nabwa_launch_dedup_heads(int n, const uint64_t *keys, uint32_t *head, hipStream_t s);
void nabwa_launch_dedup_verify(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const uint32_t *ids, const uint32_t *head,
							   int32_t *rep, uint32_t *flag, unsigned int *n_coll, hipStream_t s);
void nabwa_launch_dedup_map(int n, const int32_t *rep, const uint32_t *inner, const int64_t *off, int32_t *map, int64_t *clen, unsigned int *stat, hipStream_t s);
void nabwa_launch_dedup_compact(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const int32_t *rep, const uint32_t *inner,
								const int64_t *coff, uint8_t *cseq, uint8_t *crseq, hipStream_t s);
void nabwa_launch_dedup_expand(int n, const int32_t *map, const int32_t *n_aln, const int32_t *max_ent, const uint32_t *cent, const uint8_t *arena,
							   int32_t *n_aln_out, int32_t *max_ent_out, hipStream_t s);
/* dedup_cache_kernels.hip (dedup_cache_body.hpp): the cross-batch read cache of NABWA_DEDUP_CACHE.  lookup / map / remap run in nabwa_batch.hip's cache_lookup over the
 * n distinct reads of a batch, insert in cache_insert over the reads searched; 16 lanes per read in lookup and insert.  No kernel reads seq / rseq at or beyond off[n],
 * reads an entry beyond its size or writes the arena at or beyond arena_bytes */
void nabwa_launch_dcache_lookup(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *off, const uint64_t *hash, const uint8_t *md_tab, const uint8_t *mg_tab,
								const unsigned long long *slots, uint32_t n_slots, uint64_t mask, const uint8_t *arena, uint32_t *found, uint32_t *flag, hipStream_t s);
void nabwa_launch_dcache_map(int n, const uint32_t *found, const uint32_t *inner, const int64_t *off, int32_t *rep, int32_t *newidx, int64_t *clen, uint32_t *cent,
							 unsigned int *stat, hipStream_t s);
void nabwa_launch_dcache_remap(int n, const int32_t *old, const int32_t *newidx, int32_t *map, hipStream_t s);
void nabwa_launch_dcache_insert(int n, const uint8_t *seq, const uint8_t *rseq, const int64_t *poff, const int32_t *len, const uint8_t *rd_md, const uint8_t *rd_mg,
								const uint8_t *status, const int32_t *n_aln, const int32_t *max_ent, const uint4 *aln, int aln_cap, const int32_t *wide_idx,
								const uint4 *aln2, int aln_cap2, const uint4 *const *grown, int row_cap, uint64_t mask,
								unsigned long long *slots, uint32_t n_slots, uint8_t *arena, uint64_t arena_bytes, unsigned long long *ctr, hipStream_t s);
/* fm_deep.hip */
void nabwa_launch_fm_deep(const DeepParams *P, int n_waves, hipStream_t s);
int nabwa_deep_occupancy(int ns, int lds_rd);
/* bgzf_deflate.hip: slice k of in[0, n) -> one BGZF block at stage + k * 0x10000, its size in sizes[k]; then the blocks back to back */
void nabwa_launch_bgzf_deflate(const uint8_t *in, int64_t n, int n_slices, uint8_t *stage, uint32_t *sizes, hipStream_t s);
void nabwa_launch_bgzf_deflate_dyn(const uint8_t *in, int64_t n, int n_slices, uint8_t *stage, uint32_t *sizes, hipStream_t s);      /* dynamic Huffman blocks where they are shorter */
void nabwa_launch_bgzf_pack(const uint8_t *stage, const uint32_t *sizes, int n_slices, uint8_t *packed, int64_t *total, hipStream_t s);
/* bgzf_inflate.hip: member k (blk[k]: payload cmp + src, n_src bytes) -> isize bytes at plain + dst, its status word (bgzf_inflate_body.hpp) in status[k] */
struct BgzfInBlk;
void nabwa_launch_bgzf_inflate(const uint8_t *cmp, const struct BgzfInBlk *blk, int n_blk, uint8_t *plain, uint32_t *status, hipStream_t s);
/* finish_kernels.hip (finish_body.hpp): job t's window out of the .pac to ref + ro[t] and its query to qry + qo[t]; the alignment kernel's
 * slot-major operations (n_c32[t] of them at c32[k * n + t]) -> pos, n_cigar and a bwa_cigar_t row max_cigar wide, *n_bad += the paths
 * that do not fit; MD / NM of record t: first the length and NM, then the string at md + md_off[t] */
struct FinRef; struct FinJob; struct FinRec;
void nabwa_launch_refine_window(const uint8_t *pac, const struct FinJob *jobs, int n, const uint8_t *reads0, const uint8_t *reads1, const int64_t *ro,
								const int64_t *qo, uint8_t *ref, uint8_t *qry, hipStream_t s);
void nabwa_launch_refine_cigar(const struct FinJob *jobs, int n, int end_correct, const int32_t *n_c32, const uint32_t *c32, int max_cigar,
							   uint32_t *pos_out, int32_t *n_cigar, uint16_t *rows, unsigned int *n_bad, hipStream_t s);
void nabwa_launch_md_count(const struct FinRef *R, const struct FinRec *recs, int n, const uint8_t *reads0, const uint8_t *reads1, const uint16_t *cigar,
						   int32_t *nm, int32_t *len_out, hipStream_t s);
void nabwa_launch_md_write(const struct FinRef *R, const struct FinRec *recs, int n, const uint8_t *reads0, const uint8_t *reads1, const uint16_t *cigar,
						   const int64_t *md_off, char *md, hipStream_t s);
/* damage_kernels.hip (damage_body.hpp, rec_body.hpp): the records of *P counted into the call's table (zero before), *bad (0xffffffff before) = the lowest
 * damaged record; n_blocks workgroups share the records whatever their number.  Then the call's table onto the totals */
struct DmgParams;
void nabwa_launch_damage(const struct DmgParams *P, int n_blocks, unsigned long long *call, unsigned int *bad, hipStream_t s);
void nabwa_launch_damage_add(int words, const unsigned long long *call, unsigned long long *total, hipStream_t s);
/* markdup_kernels.hip (markdup_body.hpp, rec_body.hpp): the records of *P into the call's scratch, *bad (0xffffffff before) = the lowest damaged record;
 * then, for a sound call, their tuples onto the arena.  The resolve: the index column, the key column of the next radix pass, the marks of
 * the n sorted tuples, the marks of the n records' unmapped mates */
struct MdParams; struct MdArena;
void nabwa_launch_markdup_sig(const struct MdParams *P, int n_blocks, unsigned int *bad, hipStream_t s);
void nabwa_launch_markdup_emit(const struct MdParams *P, const struct MdArena *A, hipStream_t s);
void nabwa_launch_markdup_iota(int64_t n, uint32_t *idx, hipStream_t s);
void nabwa_launch_markdup_gather(int64_t n, const uint32_t *idx, const uint64_t *src, uint64_t *keys, hipStream_t s);
void nabwa_launch_markdup_mark(int64_t n, const uint32_t *idx, const uint64_t *hi, const uint64_t *lo, const uint64_t *k3, uint8_t *dup, unsigned long long *stats, hipStream_t s);
void nabwa_launch_markdup_prop(int64_t n, const uint8_t *link, uint8_t *dup, unsigned long long *stats, hipStream_t s);
/* bai_kernels.hip (bai_body.hpp, rec_body.hpp): the records of *P as tuples into the arena, P->cnt[0] (0xffffffff before) = the lowest damaged record,
 * P->cnt[1] (0 before) = the records without a reference.  The finish: the ordinal column, then the steps of *F in the order of the enum,
 * a sort and three scans between them (nabwa_bai.hip) */
struct BaiParams; struct BaiFin;
enum { NABWA_BAI_STEP_REF = 0, NABWA_BAI_STEP_HEAD, NABWA_BAI_STEP_PLACE, NABWA_BAI_STEP_REFSIZE, NABWA_BAI_STEP_LIN, NABWA_BAI_STEP_WRITE_REF,
	   NABWA_BAI_STEP_WRITE_TUPLE, NABWA_BAI_STEP_WRITE_LIN };
void nabwa_launch_bai_sig(const struct BaiParams *P, int n_blocks, hipStream_t s);
void nabwa_launch_bai_iota(int64_t n, uint32_t *idx, hipStream_t s);
void nabwa_launch_bai_step(int step, const struct BaiFin *F, hipStream_t s);
}
