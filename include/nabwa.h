/* include/nabwa.h -- C ABI of libnabwa.so: the MI355X-native per-read alignment hot path of
 * mpieva/network-aware-bwa, as a drop-in behind the functions `bwa bam2bam` / `bwa worker`
 * call per record.  Plain pointers and sizes only.
 *
 * All entry points return 0 on success or a negative NABWA_E* code; none falls back to a
 * CPU implementation: without a usable GPU they fail with NABWA_ENODEV.
 *
 * The reference has no FFI/plugin layer (it is one static binary), so the "binding" a
 * maintainer adds is a direct call from bam2bam.c -- shown in INTEGRATION.md.
 */
#ifndef NABWA_H
#define NABWA_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NABWA_OK        0
#define NABWA_ENODEV   -1   /* no HIP device / HIP call failed (message via nabwa_last_error) */
#define NABWA_EINVAL   -2   /* bad argument or unsupported option block */
#define NABWA_EIO      -3   /* index file missing / malformed */
#define NABWA_ENOMEM   -4
#define NABWA_ECAP     -5   /* caller-provided output capacity too small (n_aln[] / *n_rows say how much is needed) */
#define NABWA_EHITS    -6   /* some reads have more hit rows than the device-side result rows can be grown to (NABWA_ALNCAP2 = 1024 rows, searched
                             again with 16 x, 256 x, 4096 x that within NABWA_HIT_GROW_GB = 8 GB): their n_aln is 0, every other read is resolved
                             and can be fetched */
#define NABWA_EDATA    -7   /* BGZF input that is not BGZF, is cut short, or does not inflate to what its trailer says (nabwa_bgzf_decompress) */

/* gap_opt_t -- identical layout to the reference's (bwtaln.h:143-153, 64 bytes); it is the
 * block `bwa worker` receives over the wire (bam2bam.c:1260-1263). */
typedef struct {
	int s_mm, s_gapo, s_gape;
	int mode;
	int indel_end_skip, max_del_occ, max_entries;
	float fnr;
	int max_diff, max_gapo, max_gape;
	int max_seed_diff, seed_len;
	int n_threads;
	int max_top2;
	int trim_qual;
} nabwa_gap_opt_t;

#define NABWA_MODE_GAPE     0x01   /* BWA_MODE_* bits, bwtaln.h:132-141 */
#define NABWA_MODE_COMPREAD 0x02
#define NABWA_MODE_LOGGAP   0x04
#define NABWA_MODE_NONSTOP  0x10

/* bwt_aln1_t -- identical layout (bwtaln.h:41-45, 16 bytes): {n_mm:8,n_gapo:8,n_gape:8,a:1}, k, l, score */
typedef struct { uint32_t info; uint32_t k, l; int32_t score; } nabwa_aln1_t;

typedef struct nabwa_index nabwa_index_t;   /* both FM-indexes (+SA, +pac) resident in HBM */

const char *nabwa_last_error(void);
int nabwa_device_count(void);

/* gap_init_opt (bwtaln.c:19-35) */
void nabwa_gap_init_opt(nabwa_gap_opt_t *opt);
/* bwa_cal_maxdiff (bwtaln.c:37-49); host-side floating point, kept bit-compatible */
int nabwa_cal_maxdiff(int len, double err, double thres);

/* Replaces init_genome_index (bam2bam.c:844-858): reads <prefix>.bwt/.rbwt (and .sa/.rsa when
 * with_sa, .pac when with_pac) in the reference's on-disk format (bwtio.c:161-204), uploads them
 * to `device` and re-packs the Occ arrays into 64-byte buckets there.  NABWA_EINVAL for a seq_len above 0xffffffdf, or with SA samples
 * a seq_len + sa_intv above 0xffffffff: the reference's loader wraps its SA count there (bwtio.c:175). */
int nabwa_index_load(const char *prefix, int device, int with_sa, int with_pac, nabwa_index_t **out);

/* Same, from arrays already in memory (is_device != 0: device pointers on `device`).
 * bwt0/bwt1: the content of a .bwt/.rbwt file as u32 words (5 header words + Occ-interleaved BWT).
 * sa0/sa1: content of .sa/.rsa files as u32 words (7 header words + samples), or NULL. */
int nabwa_index_from_arrays(int device, int is_device, const uint32_t *bwt0, uint64_t n_words0,
							const uint32_t *bwt1, uint64_t n_words1, const uint32_t *sa0, uint64_t n_sa_words0,
							const uint32_t *sa1, uint64_t n_sa_words1, nabwa_index_t **out);
void nabwa_index_destroy(nabwa_index_t *ix);
uint32_t nabwa_index_seq_len(const nabwa_index_t *ix, int which);
uint64_t nabwa_index_device_bytes(const nabwa_index_t *ix);

/* Batch form of bwa_cal_sa_reg_gap (bwtaln.c:93-142; callers bam2bam.c:616,676, bwtaln.c:235).
 *  seq/rseq : concatenated bwa_seq_t.seq / .rseq codes (0-3, 4=N) of n reads; off[i]..off[i+1]
 *             delimit read i (seq = read reversed, rseq = its reverse complement, bwaseqio.c:294-297).
 *  per_read : !=0 gives every read the option block the reference derives when called with
 *             n_seqs==1 (bam2bam); 0 derives it once from the longest read of the batch (bwa aln).
 *  n_aln[i], max_entries[i] : as bwa_seq_t.n_aln / .max_entries.
 *  aln_out  : rows of all reads back to back in read order (capacity aln_cap rows);
 *             *n_rows receives the total.  NABWA_ECAP if aln_cap is too small (n_aln[] is still valid). */
int nabwa_cal_sa_reg_gap(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off,
						 const uint8_t *seq, const uint8_t *rseq, int per_read,
						 int32_t *n_aln, nabwa_aln1_t *aln_out, int64_t aln_cap, int64_t *n_rows,
						 int32_t *max_entries);

/* Device-resident variant for pipelines and for bench.py: upload once, run many times.
 * A batch owns the device copies of the reads, the per-lane search scratch and the outputs.
 *
 * NABWA_DEDUP (read by nabwa_batch_create, and so by everything built on it: nabwa_cal_sa_reg_gap, nabwa_bwa_cal_sa_reg_gap,
 * nabwa_bam_batch_search, the worker core, nabwa_aln, nabwa_bam2bam): unset or 0 -- every read is searched; 1 -- reads of the batch that are
 * equal in length and in every byte of seq and of rseq are found on the device and searched once; any other value is NABWA_EINVAL before any
 * device work.  What the caller sees is byte for byte what it sees without the switch: nabwa_batch_fetch (n_aln[], max_entries[], the rows in
 * the caller's read order, NABWA_ECAP with *n_rows the caller's total), nabwa_batch_checksum, nabwa_batch_width_records (first and n are the
 * caller's read indices) and nabwa_batch_config's n, min_len and max_len speak of the n reads given.  The diagnostics count the work done, that
 * is the reads searched: nabwa_batch_count_touches, *n_second_pass of nabwa_batch_sync, nabwa_batch_sure0_stats*, and cls[], n_sync and
 * hard_budget of nabwa_batch_config.  A batch without two equal reads, and one of no reads, is the batch it is without the switch.
 * NABWA_DEDUP_HASH_BITS=k (tests; 0..64, default 64, else NABWA_EINVAL; read only with NABWA_DEDUP=1): group the reads by the low k bits of
 * their hash only.  Reads that share a group and differ are searched on their own (the bytes are compared before two reads merge), so the
 * results do not change; with 0 every read shares one group.
 * With NABWA_TIMING the stage writes one line per batch to stderr: reads given, reads searched, collisions, its time by HIP events.
 *
 * NABWA_DEDUP_CACHE=<MiB> (read with NABWA_DEDUP=1, by the same entries): unset or 0 -- a batch knows nothing of earlier batches;
 * a positive number -- the index keeps, in at most that many MiB of device memory (made by the first batch that asks, out of the index's pool,
 * counted in nabwa_index_device_bytes, freed with the index; one per index, so one per replica), the results of the reads its batches searched,
 * and a later batch takes the results of a read it finds there instead of searching it.  A read is found only when its length, every byte of
 * seq and of rseq and its effective max_diff and max_gapo equal an entry's; entries are never moved or evicted, and once the cache is full
 * nothing more is entered while lookups go on.  The cache holds results of one option block at a time (every field of nabwa_gap_opt_t but
 * n_threads and trim_qual): a batch with another block empties it first when no live batch holds results from it, and goes without it
 * otherwise.  A batch that was served reads holds the cache until nabwa_batch_destroy.  What the caller sees is byte for byte what it sees
 * without the variable, with one exception: nabwa_batch_width_records returns NABWA_EINVAL for a range that holds a served read (kernel W never
 * saw it).  The diagnostics count the reads searched, as with NABWA_DEDUP; a batch all of whose reads are served searches none.
 * NABWA_EINVAL before any device work: a value that is no number or negative, a positive value without NABWA_DEDUP=1, and, for the batch that
 * makes the cache, more MiB than the device has free.  NABWA_DEDUP_HASH_BITS also narrows the key the table is probed by (the comparison does
 * not change); NABWA_DEDUP_CACHE_ROWS=<n> (default 1024, never below NABWA_ALNCAP1): reads with more hit rows are not entered. */
typedef struct nabwa_batch nabwa_batch_t;
int nabwa_batch_create(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off,
					   const uint8_t *seq, const uint8_t *rseq, int per_read, nabwa_batch_t **out);
/* enqueue the FM search of the whole batch on the batch's HIP stream (asynchronous) */
int nabwa_batch_run(nabwa_batch_t *b);
/* wait for completion; *n_second_pass = the number of reads the first pass handed on to kernel D (deep searches) */
int nabwa_batch_sync(nabwa_batch_t *b, int *n_second_pass);
/* HIP-event time of the most recent run of the dominant kernel (fm_search, first pass), ms */
float nabwa_batch_last_kernel_ms(nabwa_batch_t *b);
/* same for the width kernel (fm_width) that precedes it */
float nabwa_batch_last_width_ms(nabwa_batch_t *b);
/* same for kernel D (fm_deep: the reads the first pass handed on, one search per wavefront); 0 when it did not run */
float nabwa_batch_last_deep_ms(nabwa_batch_t *b);
/* untimed instrumented run: Occ-bucket touches the reference algorithm performs on this batch
 * (1 per bwt_occ/bwt_occ4 body, 1 per same-block bwt_2occ/bwt_2occ4), split into
 * those of bwt_match_gap (search kernel) and of the bwt_cal_width passes (width kernel) */
int nabwa_batch_count_touches(nabwa_batch_t *b, uint64_t *n_bucket, uint64_t *n_bucket_width);
int nabwa_batch_fetch(nabwa_batch_t *b, int32_t *n_aln, nabwa_aln1_t *aln_out, int64_t aln_cap, int64_t *n_rows,
					  int32_t *max_entries);
/* tests: what kernel W computes (the four bwt_cal_width passes, bwtaln.c:52-76,123-130) for reads [first, first + n): rows of
 * max_len + 1 widths and bound bytes (min(bid, 127) | (w[p-1] == w[p]) << 7) per read and strand; seed bounds seed_len + 1 wide.
 * NABWA_EINVAL when the range holds a read served from the read cache (NABWA_DEDUP_CACHE): kernel W never saw it, there are no records */
int nabwa_batch_width_records(nabwa_batch_t *b, int first, int n, uint32_t *w_out, uint8_t *bid_out, uint8_t *seed_bid_out);
/* order-independent 64-bit checksum of (read id, row index, row) over all hits, computed on the device */
int nabwa_batch_checksum(nabwa_batch_t *b, uint64_t *sum, int64_t *n_rows);
/* tests, diagnostics: what the batch-wide switches of the search came to for this batch (read-only).  -1: not decided yet
 * (n_sync, cls and hard_budget before a run, hard_budget also when kernel S does not run; coop_lanes and lds_rd while kernel D
 * has not run). */
typedef struct {
	int32_t n, min_len, max_len;
	int32_t deep_only;                        /* the option block is beyond kernel S's compact entries: every read goes to kernel D */
	int32_t ns1, ns_wide;                     /* score levels of the first pass (kernel S; computed even when deep_only) and of kernel D */
	int32_t w_sync;                           /* every read of the batch has one length: lockstep waves in kernels W and S */
	int32_t trip_budget, trip_budget_hard;    /* kernel S -> D hand-over budgets (trips) */
	int32_t n_sync;                           /* reads without an exact occurrence (kernel W's classes 1 and 2+), after a run */
	int32_t hard_budget;                      /* kernel S ran with trip_budget_hard (2 n_sync > n) */
	int32_t cls[3];                           /* reads by kernel W's class 0 / 1 / 2+, after a run */
	int32_t coop_lanes;                       /* kernel D's wave-wide one-row chains (0: off) */
	int32_t lds_rd;                           /* kernel D: bytes of one read's data in LDS (0: the read is read from HBM) */
} nabwa_batch_config_t;
int nabwa_batch_config(nabwa_batch_t *b, nabwa_batch_config_t *out);
/* tests, diagnostics: with NABWA_SURE0_STATS=1 at batch creation, what kernel S's shortcut for reads with an exact occurrence (NABWA_SURE0,
 * DESIGN.md 4) did in the runs so far: out[0] reads whose search in kernel S began with the flag set (those it later handed to kernel D included), out[1] 1-mismatch key-form children found dead in the interval table where they were created,
 * out[2] such children stored landed at table depth, out[3] reads its safety net handed to kernel D.  All 0 without the variable. */
int nabwa_batch_sure0_stats(nabwa_batch_t *b, uint64_t out[4]);
/* the same four values, then what the leap (NABWA_SURE0=3) did: out[4] leaps taken (a text-form entry that is the read's own prefix on a strand
 * that occurs exactly, replaced by its hit), out[5] levels leapt over, out[6] such entries that walked instead because their text position was
 * short of the levels left (expected 0), out[7] 0. */
int nabwa_batch_sure0_stats_ex(nabwa_batch_t *b, uint64_t out[8]);
/* tests, profiles: with NABWA_W_STATS=1, the trip counts of kernel W's last launch of this batch (nabwa_batch_run followed by nabwa_batch_sync,
 * or nabwa_batch_width_records): out[0] wave-trips, out[1] the trips of the work item that took most, out[2] text trips << 32 | their positions,
 * out[3] table trips << 32 | their positions, out[4] text trips begun in a seed pass << 32 | single steps with a rank query, out[5] single steps
 * without one (search_slots.hpp: TS_W_*; a single step is one position).  The same line goes to stderr.  All 0 without the variable. */
int nabwa_batch_w_stats(nabwa_batch_t *b, unsigned long long out[6]);
/* what NABWA_DEDUP did for this batch: out[0] reads given, out[1] reads searched, out[2] reads that shared a hash with an earlier read of the
 * batch but differ from the first read of that hash (each is searched on its own and counts in out[1]), out[3] 1 when the batch was created
 * with the switch on, else 0.  Without the switch: { n, n, 0, 0 }. */
int nabwa_batch_dedup_stats(nabwa_batch_t *b, uint64_t out[4]);
/* the same four values, then what NABWA_DEDUP_CACHE did: out[4] distinct reads served from the index's read cache (out[1] counts the others),
 * out[5] reads entered into it by nabwa_batch_sync, out[6] reads not entered (the cache full, more rows than the cap, a search that did not
 * complete, or the cache emptied for another option block meanwhile), out[7] 1 when the batch went without the cache because live batches
 * held results of another option block.  All 0 without the variable. */
int nabwa_batch_dedup_stats_ex(nabwa_batch_t *b, uint64_t out[8]);
/* the index's read cache (NABWA_DEDUP_CACHE): out[0] device bytes reserved, out[1] bytes of the entries written, out[2] entries, out[3] table
 * slots, out[4] reads looked up, out[5] reads served, out[6] times it was emptied for another option block, out[7] batches that went without
 * it.  All 0 while no batch has asked for a cache. */
int nabwa_index_dedup_cache_stats(nabwa_index_t *ix, uint64_t out[8]);
/* empties the read cache (its memory and its counts of lookups, flushes and bypasses stay); NABWA_EINVAL while a live batch holds reads
 * served from it */
int nabwa_index_dedup_cache_clear(nabwa_index_t *ix);
void nabwa_batch_destroy(nabwa_batch_t *b);

/* ---- paired-end host pieces (config 3) --------------------------------------------------------- */
/* isize_info_t without the histogram pointer (bwape.h:16-20) */
typedef struct { double avg, std, ap_prior; uint32_t low, high, high_bayesian; } nabwa_isize_t;
/* infer_isize_hist (insert_size.c:50-139) on a histogram of 100000 u16 bins; 0 = usable, -1 = not (fields as the
 * reference leaves them: avg = std = -1, bounds 0) */
int nabwa_isize_infer(const uint16_t *hist, double ap_prior, int64_t L, nabwa_isize_t *out);
/* improve_isize_est (insert_size.c:141-165): the bin a record adds one to, or -1 */
int nabwa_isize_bin(int kind, int mapq0, int mapq1, uint32_t pos0, int len0, uint32_t pos1, int len1);
/* the bwa_seq_t fields pairing() reads and writes (bwape.c:180-293) */
typedef struct { uint32_t pos; int32_t strand, mapQ, seQ, len, full_len, n_mm, n_gapo, n_gape, score, extra_flag; } nabwa_pe_end_t;
/* pairing (bwape.c:180-293; caller finish_pair, bam2bam.c:768): hits[i] = text position << 32 | hit row << 1 | end
 * for every position of every hit row of both ends (sorted in place); returns the number of moved ends with mapQ > 0 */
int nabwa_pairing(nabwa_pe_end_t p[2], int n_hits, uint64_t *hits, const nabwa_aln1_t *rows0, const nabwa_aln1_t *rows1,
				  int max_isize, int s_mm, const nabwa_isize_t *ii);

/* ---- the reference's own record struct ------------------------------------------------------ */
/* bwa_seq_t (bwtaln.h:64-90), 200 bytes; bit-fields kept as the words the compiler packs them into:
 * bits0 = len:20 | strand:1 | type:2 | dummy:1 | extra_flag:8 ; bits1 = n_mm:8 | n_gapo:8 | n_gape:8 | mapQ:8 ;
 * c1c2seq = c1:28 | c2:28 | seQ:8 ; lenbits = full_len:20 | nm:12 */
typedef struct {
	char *name;
	uint8_t *seq, *rseq, *qual;
	uint32_t bits0, bits1;
	int32_t score, clip_len;
	int32_t n_aln; int32_t pad0;
	nabwa_aln1_t *aln;
	int32_t n_multi; int32_t pad1;
	void *multi;
	uint32_t sa, pos;
	uint64_t c1c2seq;
	int32_t n_cigar; int32_t pad2;
	uint16_t *cigar;
	int32_t tid;
	char bc[64];
	uint32_t lenbits;
	char *md;
	int32_t max_entries; int32_t pad3;
} nabwa_bwa_seq_t;

/* Drop-in for bwa_cal_sa_reg_gap(bwt, n_seqs, seqs, opt) (bwtaln.h:187; callers bam2bam.c:616,676, bwtaln.c:235)
 * on the reference's own records. */
int nabwa_bwa_cal_sa_reg_gap(nabwa_index_t *ix, int n_seqs, nabwa_bwa_seq_t *seqs, const nabwa_gap_opt_t *opt);

/* The encoding half of bam1_to_seq (bwaseqio.c:272-307) incl. seq_reverse (:91-108) and bwa_trim_read (:110-123):
 * codes = bases of the BAM record (0-3, 4 = N), qual = phred values or NULL; returns the (trimmed) length and fills
 * seq_out (read reversed) and rseq_out (its complement, i.e. the reverse complement of the read). */
int nabwa_encode_read(int full_len, const uint8_t *codes, const uint8_t *qual, int reverse, int trim_qual, int is_comp,
					  uint8_t *seq_out, uint8_t *rseq_out);

/* Batch form of bwt_sa (bwt.c:72-81; callers bam2bam.c:635-636,752,761,786, bwase.c:146,151):
 * sa_out[i] = SA value of row k[i] in index `which[i]` (0 forward, 1 reversed text). */
int nabwa_sa_lookup(nabwa_index_t *ix, int n, const uint8_t *which, const uint32_t *k, uint32_t *sa_out);

/* Batch form of aln_global_core + aln_path2cigar32 (stdaln.c:345-525, :1009-1039; caller
 * refine_gapped_core, bwase.c:212): task i aligns ref[ref_off[i]..ref_off[i+1]) (seq1) with
 * qry[qry_off[i]..qry_off[i+1]) (seq2), codes 0-4, under {gap_open, gap_ext, gap_end, 5x5 matrix,
 * band_width} (AlnParam, stdaln.h:86-95).  cigar32 rows are max_cigar wide (len<<4 | op);
 * n_cigar[i] > max_cigar means the row was truncated. */
int nabwa_global_align(int device, int n, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off,
					   const uint8_t *qry, int gap_open, int gap_ext, int gap_end, const int *matrix25, int band,
					   int32_t *score, int32_t *n_cigar, uint32_t *cigar32, int max_cigar);

/* The alignment entry points keep their device working memory (score rows, traceback matrices) between calls; this frees it. */
void nabwa_dp_scratch_release(int device);

/* tests, diagnostics: launches of the alignment kernels by form since the library was loaded, each picked per launch from the
 * batch's largest task: [0] global, one wavefront per task; [1] global, lanes with rows in LDS; [2] global, lanes with rows in
 * HBM; [3] local, rows in LDS; [4] local, rows in HBM; [5] extension, rows in LDS; [6] extension, rows in HBM.  Writes min(n, 7)
 * counts. */
void nabwa_dp_form_counts(uint64_t *out, int n);

/* Batch form of aln_extend_core (stdaln.c:862-1007): left-anchored extension seeded with G0[i], then the
 * path by global alignment of the two prefixes (gap_end = -1, band doubled until the scores agree or it
 * exceeds the prefix lengths).  score[i] as the reference returns it (<= 0: no extension, n_cigar 0). */
int nabwa_extend_align(int device, int n, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off,
					   const uint8_t *qry, int gap_open, int gap_ext, const int *matrix25, int band, const int32_t *G0,
					   int32_t *score, int32_t *n_cigar, uint32_t *cigar32, int max_cigar);

/* Batch form of aln_local_core (stdaln.c:529-761; caller bwa_sw_core, bwape.c:456, mate rescue) with
 * _thres = thres > 0: forward and reverse Smith-Waterman passes, then the path by global alignment of the
 * sub-matrix (gap_end = -1, doubling band).  coords rows: start_i, start_j, end_i, end_j (1-based);
 * subo (may be NULL): sub-optimal score as stdaln.c:700-709. */
int nabwa_local_align(int device, int n, const int64_t *ref_off, const uint8_t *ref, const int64_t *qry_off,
					  const uint8_t *qry, int gap_open, int gap_ext, const int *matrix25, int band, int thres,
					  int32_t *score, int32_t *coords, int32_t *subo, int32_t *n_cigar, uint32_t *cigar32, int max_cigar);

/* ---- single-end finishing chain: everything between the FM search and the BAM record -------- */
#define NABWA_MAX_CIGAR 64
#define NABWA_MAX_MD    512
#define NABWA_MAX_MULTI 16
typedef struct { uint32_t pos; int32_t gap, mm, strand, n_cigar; uint16_t cigar[NABWA_MAX_CIGAR]; } nabwa_multi_t;
typedef struct {
	int32_t type, strand, n_mm, n_gapo, n_gape, score;     /* bwa_seq_t fields of the same names (bwtaln.h:64-90) */
	uint32_t sa, pos, c1, c2;
	int32_t mapQ, seQ, len, full_len, clip_len;
	int32_t n_cigar; uint16_t cigar[NABWA_MAX_CIGAR];       /* bwa_cigar_t: op<<14 | len (bwtaln.h:47-56) */
	int32_t nm; char md[NABWA_MAX_MD];
	int32_t n_multi; nabwa_multi_t multi[NABWA_MAX_MULTI];
	/* what bwa_print_sam1 / bwa_update_bam1 derive (bwase.c:458-571, bam2bam.c:430-593) */
	int32_t flag, seqid, nn; int64_t rpos; char xt;
} nabwa_se_t;

/* Annotation side of the index (replaces bns_restore + bwt_restore_pac, bntseq.c:88-148): <prefix>.ann,
 * .amb and .pac are read into host memory and attached to the index. */
int nabwa_index_attach_reference(nabwa_index_t *ix, const char *prefix);
/* what bns_restore read (bntseq.c:88-139): contigs (name, offset in the concatenated reference, length), total length, srand48 seed */
int nabwa_index_n_contigs(const nabwa_index_t *ix);
int nabwa_index_contig(const nabwa_index_t *ix, int i, char *name, int name_cap, int64_t *offset, int32_t *len);
int nabwa_index_reference_info(const nabwa_index_t *ix, int64_t *l_pac, uint32_t *seed);
/* the same from memory (bntseq_t: contigs with offsets and lengths, bntamb1_t holes, the .pac bytes) */
int nabwa_index_set_reference(nabwa_index_t *ix, int64_t l_pac, uint32_t seed, int n_seqs, const char *const *names,
							  const int64_t *offsets, const int32_t *lens, int n_holes, const int64_t *hole_off,
							  const int32_t *hole_len, const char *hole_amb, const uint8_t *pac);

/* bwa_aln2seq_core (bwase.c:19-95) -> bwa_cal_pac_pos_core + multi-hit positions (bwase.c:139-181,
 * bam2bam.c:629-637) -> bwa_refine_gapped (bwase.c:356-423: gap refinement, MD/NM, trimmed-tail clip) for
 * n single-end reads IN RECORD ORDER.  The hit choice consumes the caller's drand48 stream: *rng48 is the
 * 48-bit state (srand48(seed) == ((uint64_t)seed << 16) | 0x330E) and is updated, so that successive
 * batches continue the reference's process-global stream.  SA lookups and the gap-refinement
 * DP run on the GPU in batches; the rest is host bookkeeping.
 * full_len[i] >= len: untrimmed read length (bwa_seq_t.full_len).  n_occ: max_occ_se (bam2bam.c:629; <= 15). */
int nabwa_se_finish(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const uint8_t *seq,
					const uint8_t *rseq, const int32_t *full_len, const int32_t *n_aln, const nabwa_aln1_t *aln,
					int n_occ, uint64_t *rng48, nabwa_se_t *out);

/* The two halves of nabwa_se_finish on their own, as bam2bam's two passes need them:
 * nabwa_se_posn   = posn_singleton (bam2bam.c:622-641): hit choice on the caller's drand48 stream, bwt_sa batch, mapQ;
 * nabwa_se_refine = bwa_refine_gapped (bwase.c:356-423; finish_singleton, bam2bam.c:643-651) on positioned records + the
 *                   flag / contig / XT fields bwa_update_bam1 derives.  NABWA_ECAP if an MD string exceeds NABWA_MAX_MD. */
int nabwa_se_posn(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
				  const int32_t *n_aln, const nabwa_aln1_t *aln, int n_occ, uint64_t *rng48, nabwa_se_t *out);
int nabwa_se_refine(nabwa_index_t *ix, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, nabwa_se_t *inout);
/* nabwa_se_posn with a hit-list bound per read (singletons: max_occ_se, ends of pairs: 0 -- one drand48 stream for a mixed file) */
int nabwa_se_posn_v(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const int32_t *full_len,
					const int32_t *n_aln, const nabwa_aln1_t *aln, const uint8_t *n_occ_v, uint64_t *rng48, nabwa_se_t *out);

/* ---- the finishing chains' device path ----------------------------------------------------------
 * NABWA_FINISH (read at every call of a chain: nabwa_se_refine, nabwa_se_finish, nabwa_se_finish_cs, nabwa_pe_finish* and what is built on
 * them): unset or `host` = the reference windows, the CIGAR end rules and MD / NM on host threads; `gpu` = on the device, with the 2-bit
 * reference and its ambiguity holes held in HBM (uploaded by the first call that needs them, l_pac / 4 + 1 bytes, counted in
 * nabwa_index_device_bytes); anything else: NABWA_EINVAL.  The records are the same either way.  The two per-record functions of
 * bwa_refine_gapped as batches, for an integrator who keeps the loop of bwase.c:356-423 (which_ref: 0 = the reference of
 * nabwa_index_attach_reference, 1 = the nucleotide reference of a colour index, nabwa_index_attach_nt_reference): */
/* Batch form of refine_gapped_core (bwase.c:189-237) with aln_param_bwa: job i refines query qry[qry_off[i]..qry_off[i+1]) (codes 0-4,
 * alignment orientation) at pos[i] with ext[i] = +gaps on the reverse strand, -gaps on the forward one.  pos is updated; cigar rows are
 * max_cigar wide, bwa_cigar_t.  NABWA_ECAP if a path needs more operations than max_cigar. */
int nabwa_refine_gapped_core(nabwa_index_t *ix, int which_ref, int is_end_correct, int n, const int64_t *qry_off, const uint8_t *qry,
                             const int32_t *ext, uint32_t *pos, int32_t *n_cigar, uint16_t *cigar, int max_cigar);
/* Batch form of bwa_cal_md1 (bwase.c:253-315): n_cigar[i] == 0 is the ungapped branch.  md: strings back to back, each NUL-terminated,
 * record i at md_off[i]; NABWA_ECAP with md_off[n] = bytes needed when md_cap is too small. */
int nabwa_cal_md(nabwa_index_t *ix, int which_ref, int n, const int64_t *qry_off, const uint8_t *qry, const uint32_t *pos,
                 const int32_t *n_cigar, const uint16_t *cigar, int max_cigar, int32_t *nm, int64_t *md_off, char *md, int64_t md_cap);
/* Both: NABWA_EINVAL for a null argument, for no attached reference (or no nucleotide reference when which_ref is 1), for a query length
 * outside 1 .. 0x3fff, an ext outside -0xffff .. 0xffff or a query code above 4 (nabwa_refine_gapped_core), for a CIGAR that does not
 * consume its query exactly, and for an ungapped nabwa_cal_md record with pos + len > l_pac (the reference reads outside its array there);
 * NABWA_ENODEV without a device: there is no CPU fallback. */
/* tests, diagnostics: since the library was loaded -- [0] jobs refined by nabwa_refine_gapped_core or the chains' device path,
 * [1] records whose MD / NM the device wrote, [2] calls of a chain that took the device path, [3] bytes of reference held in HBM for it */
void nabwa_finish_counts(uint64_t out[4]);

/* ---- paired-end chain (config 3) ------------------------------------------------------------ */
/* pe_opt_t (bwtaln.h:158-164), same layout; defaults as bwa_init_pe_opt (bwape.c:27-41) */
typedef struct {
	int32_t max_isize, force_isize, max_occ, max_occ_se, n_multi, N_multi, type, is_sw, is_preload;
	double ap_prior;
} nabwa_pe_opt_t;
void nabwa_pe_opt_default(nabwa_pe_opt_t *po);

/* one end of a pair: the single-end record plus what bwa_update_bam1 derives from the mate (bam2bam.c:430-525).
 * se.flag is the final SAM flag; extra_flag is bwa_seq_t.extra_flag (paired / read1 / read2 / proper pair). */
typedef struct {
	nabwa_se_t se;
	int32_t extra_flag, m_seqid, am;
	int32_t mapQ_paired;                                   /* se.mapQ as pairing left it; se.mapQ itself is cleared when the hit bridges two contigs (bam2bam.c:453-458) */
	int64_t m_rpos, isize;                                 /* mate position (1-based, on contig m_seqid), template length */
} nabwa_pe_t;

/* posn_pair (bam2bam.c:683-703) for n_pairs pairs: bwa_aln2seq + bwa_cal_pac_pos_core per end, IN RECORD ORDER
 * (pair 0 end 0, pair 0 end 1, pair 1 end 0, ...) on the caller's drand48 stream.  Reads, hit rows and records
 * are interleaved: index 2*pair + end.  Afterwards the caller bins insert sizes (nabwa_isize_bin on pos / len /
 * mapQ of the two ends) and, once all batches are in, calls nabwa_isize_infer -- the barrier of bam2bam. */
int nabwa_pe_posn(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n_pairs, const int64_t *off, const int32_t *full_len,
				  const int32_t *n_aln, const nabwa_aln1_t *aln, uint64_t *rng48, nabwa_pe_t *out);

/* finish_pair (bam2bam.c:705-811) for the same pairs: hit enumeration (bwt_sa, GPU batch) + pairing (bwape.c:180-293),
 * multi-hit lists, mate rescue (bwa_paired_sw1 / bwa_sw_core, bwape.c:433-633; local alignments as one GPU batch),
 * bwa_refine_gapped on both ends (global alignments as one GPU batch), MD / NM, flags and mate fields.
 * ii: the read group's insert-size estimate; all zeros = none (null_ii, bam2bam.c:715).
 * n_tot / n_mapped (may be NULL): the counters of bwa_paired_sw1, [0] discordant pairs, [1] singletons. */
/* improve_isize_est (insert_size.c:141-165) for the positioned pairs of one batch: hist = 100000 uint16_t bins, wrapping as the
 * reference's do; call between nabwa_pe_posn and nabwa_isize_infer */
int nabwa_isize_add_pairs(int n_pairs, const nabwa_pe_t *recs, uint16_t *hist);
int nabwa_pe_finish(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const nabwa_isize_t *ii,
					int n_pairs, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, const int32_t *n_aln,
					const nabwa_aln1_t *aln, nabwa_pe_t *inout, uint64_t n_tot[2], uint64_t n_mapped[2]);
/* finish_pair's per-file position cache (kh_64_t *my_hash, bam2bam.c:707,741-757; one per pass 2 in `bam2bam -t 1`, :1186-1203): hit rows of
 * MIN_HASH_WIDTH = 1000 suffixes or more get their text positions once per file, under the key (k, l) alone -- later reads with the same
 * row take the positions of the first read that brought it, computed with THAT read's strand and length.  Pass the same cache to every
 * batch of a file, batches in input order, to get what the sequential reference writes; NULL = every row on its own (a cold cache). */
typedef struct nabwa_poscache nabwa_poscache_t;
nabwa_poscache_t *nabwa_poscache_create(void);
void nabwa_poscache_destroy(nabwa_poscache_t *c);
int64_t nabwa_poscache_size(const nabwa_poscache_t *c);      /* rows entered so far */
int nabwa_pe_finish_cached(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const nabwa_isize_t *ii,
						   int n_pairs, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, const int32_t *n_aln,
						   const nabwa_aln1_t *aln, nabwa_pe_t *inout, uint64_t n_tot[2], uint64_t n_mapped[2], nabwa_poscache_t *cache);

/* ---- the same phases on the reference's own records (bwa_seq_t), one call per phase and batch ---------------------
 * Each replaces the per-record function of the same role in bam2bam.c; fields are left as that function leaves them, and
 * multi / multi[].cigar / cigar / md are malloc'd for bwa_free_read_seq1 (bwaseqio.c:253-261) to free.
 *   nabwa_bwa_posn_se       posn_singleton (bam2bam.c:622-641): bwa_aln2seq_core(.., 1, max_occ_se), bwa_cal_pac_pos_core, multi positions
 *   nabwa_bwa_refine_gapped bwa_refine_gapped(bns, n, seqs, pac, ntbns) (bwase.h:16; bam2bam.c:649,799-800), seq un-reversed as there
 *   nabwa_bwa_posn_pe       posn_pair (bam2bam.c:683-703); records interleaved, 2 * pair + end
 *   nabwa_bwa_finish_pe     finish_pair up to bwa_update_bam1 (bam2bam.c:705-800): pairing (bwape.h:46), bwa_paired_sw1 (bwape.h:49),
 *                           multi lists, bwa_refine_gapped on both ends
 * rng48: the drand48 state (srand48(seed) == ((uint64_t)seed << 16) | 0x330E), consumed in record order. */
int nabwa_bwa_posn_se(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int max_occ_se, int n, nabwa_bwa_seq_t *seqs, uint64_t *rng48);
int nabwa_bwa_refine_gapped(nabwa_index_t *ix, int n, nabwa_bwa_seq_t *seqs);
int nabwa_bwa_posn_pe(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n_pairs, nabwa_bwa_seq_t *seqs, uint64_t *rng48);
int nabwa_bwa_finish_pe(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const nabwa_isize_t *ii,
						int n_pairs, nabwa_bwa_seq_t *seqs, uint64_t n_tot[2], uint64_t n_mapped[2]);
/* the same with finish_pair's my_hash argument (bam2bam.c:707): one cache per pass 2 of a file */
int nabwa_bwa_finish_pe_cached(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const nabwa_isize_t *ii,
							   int n_pairs, nabwa_bwa_seq_t *seqs, uint64_t n_tot[2], uint64_t n_mapped[2], nabwa_poscache_t *cache);

/* ---- the batching front-end: BAM records in, BAM records out (what sits behind `bwa bam2bam` / `bwa worker`) --------
 * A batch = n_rec records as they stand in an uncompressed BAM stream (u32 block_size + block), in file order, mates adjacent.
 *   create : read_bam_pair's record logic (bwaseqio.c:340-494: singleton / pair, QC flag over mates, erase_unwanted_tags) and
 *            bam1_to_seq (bwaseqio.c:272-307)
 *   pass1  : pair_aln + pair_posn + improve_isize_est per logical record, in record order on the caller's drand48 stream
 *            (bam2bam.c:1143-1176, 608-703; insert_size.c:141-165)
 *   pass2  : pair_finish incl. bwa_update_bam1 (bam2bam.c:1178-1216, 643-658, 705-811, 430-593), each read group with its
 *            own insert-size estimate
 *   output : the records (uncompressed BAM bytes; BGZF and the header are the caller's, as they are bam2bam's own bgzf.c)
 * Between the passes of ALL batches: nabwa_isize_table_infer_all (infer_all_isizes, insert_size.c:167-173). */
typedef struct nabwa_isize_table nabwa_isize_table_t;
typedef struct nabwa_bam_batch nabwa_bam_batch_t;
nabwa_isize_table_t *nabwa_isize_table_create(double ap_prior, int64_t genome_len);
void nabwa_isize_table_destroy(nabwa_isize_table_t *t);
int nabwa_isize_table_infer_all(nabwa_isize_table_t *t);
/* the estimate of a read group; returns 1 and all zeros (null_ii, bam2bam.c:106) when it has none */
int nabwa_isize_table_get(const nabwa_isize_table_t *t, const char *rg, nabwa_isize_t *out);
/* histograms of another shard's pass 1 added in (N GPUs: the one cross-shard reduction of the pipeline) */
int nabwa_isize_table_merge(nabwa_isize_table_t *t, const nabwa_isize_table_t *other);
/* encode_iinfo / decode_iinfo (insert_size.c:185-213): the blob a `bwa worker` is sent; encode returns the size needed */
int64_t nabwa_isize_table_encode(const nabwa_isize_table_t *t, uint8_t *out, int64_t cap);
int nabwa_isize_table_decode(nabwa_isize_table_t *t, const uint8_t *in, int64_t n);
int nabwa_bam_batch_create(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, int n_rec,
						   const uint8_t *in, const int64_t *in_off, nabwa_bam_batch_t **out);
/* the same with bam2bam's record-handling switches (bam2bam.c:96-101,1988-1993):
 *   BROKEN_INPUT    --broken-input   : read_bam_pair's allow_broken (bwaseqio.c:345-410): wrong read 1 / read 2 flags of two reads of
 *                                      one name are set right, a paired read followed by another name (or by nothing) is discarded
 *   DROP_ALIGNED    --drop-aligned   : logical records with a read that is already mapped are left out (bwaseqio.c:466-474)
 *   SKIP_DUPLICATES --skip-duplicates: logical records with a read flagged as duplicate (0x400) are neither aligned nor counted
 *                                      for the insert size; they come out as they came in, less the erased tags (unique(), bam2bam.c:595-606)
 *   DEBUG           --debug-bam      : YQ:i = the most entries the search of the read held (bam2bam.c:433)
 *   ONLY_ALIGNED    --only-aligned   : output leaves out logical records with a read that stayed unmapped (pair_print_bam, bam2bam.c:911-925) */
#define NABWA_BAM_BROKEN_INPUT    1u
#define NABWA_BAM_DROP_ALIGNED    2u
#define NABWA_BAM_SKIP_DUPLICATES 4u
#define NABWA_BAM_DEBUG           8u
#define NABWA_BAM_ONLY_ALIGNED    16u
#define NABWA_BAM_ALL_FLAGS       31u
int nabwa_bam_batch_create_ex(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, uint32_t flags, int n_rec,
							  const uint8_t *in, const int64_t *in_off, nabwa_bam_batch_t **out);
/* optional, before pass 1 and from any thread: the FM search of the batch (the part of pass 1 that needs neither the random stream
 * nor the batches before it) on the GPU of the index the batch was created with; pass 1 then goes on from its rows.  This is how
 * one process keeps several GPUs busy: batches are dealt to index replicas, searched as they come, and passed in input order. */
int nabwa_bam_batch_search(nabwa_bam_batch_t *b);
int nabwa_bam_batch_pass1(nabwa_bam_batch_t *b, uint64_t *rng48, nabwa_isize_table_t *tab);
/* pass 2 keeps finish_pair's position cache (above) in the table: the batches of a file pass in input order, as the records of
 * `bam2bam -t 1` do */
int nabwa_bam_batch_pass2(nabwa_bam_batch_t *b, const nabwa_isize_table_t *tab, uint64_t n_tot[2], uint64_t n_mapped[2]);
int nabwa_bam_batch_output(const nabwa_bam_batch_t *b, uint8_t *out, int64_t cap, int64_t *out_off, int64_t *n_bytes);
int nabwa_bam_batch_counts(const nabwa_bam_batch_t *b, int *n_records, int *n_logical);
/* per logical record: 1 (a single read) or 2 (a pair); n_logical entries */
int nabwa_bam_batch_kinds(const nabwa_bam_batch_t *b, uint8_t *kind_out);
void nabwa_bam_batch_destroy(nabwa_bam_batch_t *b);

/* ---- 0MQ worker compatibility: the wire record, and a worker core that is independent of the transport ----------
 * `bwa bam2bam -p PORT` hands logical records to `bwa worker` processes as 0MQ messages and takes them back one phase further
 * (run_worker_thread, bam2bam.c:1387-1442); the same bytes, with a u32 length in front, are the records of its temporary file
 * between the passes (pair_print_custom / read_pair_custom, bam2bam.c:1099-1135).  One message (msg_init_from_pair, bam2bam.c:951-1006;
 * inverse pair_init_from_msg, :1040-1097):
 *    u64 recno (little endian) . u8 kind (0 end marker, 1 single read, 2 pair) . u8 phase (0 pristine, 1 aligned, 2 positioned, 3 finished)
 *    per read:  bam1_core_t as the HOST lays it out, 32 bytes (bamlite.h:44-53: word 2 = bin | qual << 16 | l_qname << 24, word 3 =
 *               flag | n_cigar << 16 -- not the order of a BAM file) . i32 data_len . data (name, CIGAR, bases, qualities, tags)
 *      phase positioned:  u8 strand << 4 | type . u8 n_mm, n_gapo, n_gape, seQ, mapQ . i32 len, clip_len, score, sa, c1, c2, pos, n_multi .
 *                         n_multi raw bwt_multi1_t of 16 bytes (u32 pos . u32 n_cigar:15 | gap:8 | mm:8 | strand:1 . a dead pointer)
 *      phases aligned, positioned:  i32 max_entries . i32 n_aln . n_aln raw bwt_aln1_t of 16 bytes
 * Parity unpinned: libzmq is absent from the image and bam2bam.c cannot be compiled, so no byte of a reference message exists to compare
 * with; the codec follows the cited lines, and tests/test_wire.py builds messages by hand from them. */
#define NABWA_KIND_EOF 0
#define NABWA_KIND_SINGLE 1
#define NABWA_KIND_PAIR 2
#define NABWA_PHASE_PRISTINE 0
#define NABWA_PHASE_ALIGNED 1
#define NABWA_PHASE_POSITIONED 2
#define NABWA_PHASE_FINISHED 3
typedef struct {
	uint8_t core[32];                       /* bam1_core_t, host layout */
	int32_t data_len; const uint8_t *data;  /* bam1_t.data */
	uint8_t strand, type, n_mm, n_gapo, n_gape, seQ, mapQ;                 /* positioned */
	int32_t len, clip_len, score; uint32_t sa, c1, c2, pos;
	int32_t n_multi; const uint8_t *multi;                                 /* n_multi x 16 raw bytes (may be unaligned) */
	int32_t max_entries, n_aln; const uint8_t *aln;                        /* aligned, positioned: n_aln x 16 raw bytes (may be unaligned) */
} nabwa_wire_read_t;
typedef struct { uint64_t recno; uint8_t kind, phase; nabwa_wire_read_t read[2]; } nabwa_wire_rec_t;
/* bytes the message of r takes */
int64_t nabwa_wire_size(const nabwa_wire_rec_t *r);
/* msg_init_from_pair: writes the message, returns its size; NABWA_ECAP if cap is too small, NABWA_EINVAL for a kind / phase that does not exist */
int64_t nabwa_wire_encode(const nabwa_wire_rec_t *r, uint8_t *out, int64_t cap);
/* pair_init_from_msg: the pointers of *out point into msg.  NABWA_EINVAL unless the message is consumed exactly (the reference exits there) */
int nabwa_wire_decode(const uint8_t *msg, int64_t len, nabwa_wire_rec_t *out);
/* a record as it stands in a BAM stream (u32 block_size, 32 bytes of core in file order, data) <-> core in host layout + data */
void nabwa_wire_core_from_bam(const uint8_t bam_core[32], uint8_t wire_core[32]);
void nabwa_wire_core_to_bam(const uint8_t wire_core[32], uint8_t bam_core[32]);
/* the reply to a worker's hello (run_config_service, bam2bam.c:1255-1266; read at :2260-2274): gap_opt_t . pe_opt_t . index prefix, not terminated */
int64_t nabwa_wire_config_encode(const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const char *prefix, uint8_t *out, int64_t cap);
int nabwa_wire_config_decode(const uint8_t *msg, int64_t len, nabwa_gap_opt_t *opt, nabwa_pe_opt_t *popt, char *prefix, int prefix_cap);

/* The state pass 1 leaves a batch in, read by read, and the way back: what lets a positioned record leave the process (the temporary
 * file between the passes, a worker's reply) and come back into a fresh batch made from the same records.
 *   nabwa_bam_batch_positioned : after pass 1; fills the positioned and aligned parts of out[0 .. n_records) (core / data are left alone),
 *                                pointers into the batch, valid until it is destroyed
 *   nabwa_bam_batch_restore    : on a batch just created from the same records: takes the state from in[0 .. n_records) instead of
 *                                searching and positioning; the batch is then where pass 1 would have left it (no random numbers drawn, no
 *                                insert sizes counted).  NABWA_EINVAL if a read's length disagrees with the batch's (other trimming options). */
int nabwa_bam_batch_positioned(nabwa_bam_batch_t *b, nabwa_wire_read_t *out);
int nabwa_bam_batch_restore(nabwa_bam_batch_t *b, const nabwa_wire_read_t *in);

/* The worker's side of the exchange without a socket in sight: messages in, messages out.
 *   pristine / aligned records : pair_aln + pair_posn (bam2bam.c:1414-1416) on the worker's own drand48 stream in arrival order
 *                                (srand48(bns->seed) at start, bam2bam.c:2284) -> positioned
 *   positioned records         : pair_finish with the insert-size estimates last set (bam2bam.c:1419) -> finished; without estimates the
 *                                record goes back as it came and counts as a failure (1024 of them end the worker, :1428-1433)
 *   finished records, end markers: go back as they came
 * Records are gathered into batches for the GPU; replies leave in arrival order.  A record sent twice (the master's resend loop,
 * bam2bam.c:1587-1596) is simply worked on twice, as the reference's workers do -- nothing is remembered between messages but the
 * random stream, the estimates and finish_pair's position cache. */
typedef struct nabwa_worker nabwa_worker_t;
int nabwa_worker_create(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, nabwa_worker_t **out);
void nabwa_worker_destroy(nabwa_worker_t *w);
/* the insert-size broadcast (`\2` + blob, handle_broadcast, bam2bam.c:2079-2097) or the reply to `\1nodename` (:2286-2299): decode_iinfo's blob */
int nabwa_worker_set_isize(nabwa_worker_t *w, const uint8_t *blob, int64_t n);
typedef int (*nabwa_send_fn)(void *ctx, const uint8_t *msg, int64_t len);                               /* 0 = sent */
/* returns 1 with a message (valid until the next call), 0 when none came within timeout_ms, -1 when the transport is closed */
typedef int (*nabwa_recv_fn)(void *ctx, const uint8_t **msg, int64_t *len, int timeout_ms);
/* one batch of messages: every one is answered through send, in the order given */
int nabwa_worker_process(nabwa_worker_t *w, int n_msg, const uint8_t *const *msgs, const int64_t *lens, nabwa_send_fn send, void *ctx);
/* bwa_worker_core's loop (bam2bam.c:2099-2176) over a transport: gathers up to max_batch messages (waiting linger_ms for more once one
 * is there), processes them, goes on; returns NABWA_OK when nothing came for idle_timeout_ms (the reference: 90 s) or the transport closed,
 * NABWA_EIO after 1024 positioned records without estimates */
typedef struct { int32_t max_batch, linger_ms, idle_timeout_ms; } nabwa_worker_opt_t;
int nabwa_worker_core(nabwa_worker_t *w, nabwa_recv_fn recv, nabwa_send_fn send, void *ctx, const nabwa_worker_opt_t *wo);
/* counters: records positioned, finished, bounced (no estimates), passed through */
void nabwa_worker_counts(const nabwa_worker_t *w, uint64_t out[4]);

/* Read-back of the index parts derived at load time (tests): what 0 = full SA, 1 = inverse SA, 2 = text bases (one per
 * word), 3 = interval-table entries {k, l} of the last level (two words per key), 4 = the table's depth T (one word),
 * 5 = the primary keys of table levels first.. (levels 0..16, one word each: the key whose interval holds the primary row, ~0u = none). */
int nabwa_index_export(const nabwa_index_t *ix, int which, int what, uint64_t first, uint64_t n, uint32_t *out);

/* Rank primitives for tests: Occ of all four bases at rows k[i] (bwt_occ4, bwt.c:159-176). */
int nabwa_occ4(nabwa_index_t *ix, int which, int n, const uint32_t *k, uint32_t *cnt_out /* n x 4 */);

/* ---- index construction: `bwa index` (bwtindex.c:39-196) ------------------------------------------------------------
 * nabwa_index_fa2pac   = bns_fasta2bntseq + bns_dump (bntseq.c:58-85,166-256) and bwa_pac_rev_core (bwtmisc.c:168-193): FASTA or
 *                        FASTQ, plain or gzip, in; <prefix>.pac, .ann, .amb and .rpac out, byte for byte the reference's (ambiguous
 *                        bases drawn from lrand48 after srand48(11), holes, the stale-comment quirk of kseq).  Host only, no GPU.
 *                        Returns l_pac, or a negative NABWA_E*: NABWA_EINVAL for an input without bases or over 4 Gbp (nothing is
 *                        written then; "over 4 Gbp" means over 4 294 967 168 bases, 0xffffff80, where the reference's own Occ count
 *                        wraps, bwtmisc.c:131), NABWA_EIO for a file that cannot be read or written.  prefix NULL: read and check the
 *                        input only, write nothing.
 * nabwa_index_fa2cspac = the same for `bwa index -c` (bwtindex.c:84-98, bwa_pac2cspac, bwtmisc.c:210-254): <prefix>.nt.pac/.ann/.amb
 *                        of the bases, then the colour text as <prefix>.pac/.ann/.amb/.rpac.  Host only.
 * nabwa_index_build    = the BWT, Occ and SA steps (bwtindex.c:104-191) on the GPU: <prefix>.pac in, <prefix>.bwt, .rbwt (of the
 *                        reversed text), .sa and .rsa (every sa_intv-th row; the reference uses 32) out, the words the reference writes
 *                        whichever of -a is / bwtsw it runs.  The worst-case device memory (nabwa_index_build_estimate, about
 *                        41 bytes per base) is checked against the device's free memory and against NABWA_INDEX_MAX_BYTES when that
 *                        is set: NABWA_ENOMEM before any allocation if it does not fit.  Texts up to 4 294 967 168 bases
 *                        (0xffffff80, as nabwa_index_fa2pac); a longer .pac is NABWA_EINVAL before its bases are read, and so is
 *                        an sa_intv with l_pac + sa_intv > 0xffffffff (the reference's loader would wrap n_sa, bwtio.c:175).
 *                        verbose != 0: stage times and peak device memory on stderr. */
int64_t nabwa_index_fa2pac(const char *fasta, const char *prefix);
int64_t nabwa_index_fa2cspac(const char *fasta, const char *prefix);
int nabwa_index_build(const char *prefix, int device, int sa_intv, int verbose);
int nabwa_index_build_estimate(uint64_t l_pac, uint64_t *bytes);

/* ---- `bwa samse` / `bwa sampe` (bwase.c:595-750, bwape.c:655-817): the pieces the bam2bam chain above does not share ----------
 * nabwa_isize_infer_pairs = infer_isize (bwape.c:74-175) over ONE chunk of n_pairs positioned pairs; pos / len / mapq are indexed
 *                           2 * pair + end (as nabwa_pe_posn leaves its records).  A pair counts when both ends have mapQ >= 20 and
 *                           its outer distance is below 100000; low is floored at the longest read of the chunk; the doubles follow
 *                           the reference's order of operations.  Returns 0, NABWA_ISIZE_FEW (fewer than 20 good pairs) or
 *                           NABWA_ISIZE_WEIRD (std is NaN or the 75th percentile is over 100000); on both failures avg = std = -1 and
 *                           the bounds are 0, ap_prior is the given prior (too few) or the estimate's (weird).  log (may be NULL): the reference's `[infer_isize] ...` stderr lines, NUL-terminated,
 *                           cut at log_cap bytes.
 * nabwa_pe_finish_sampe   = nabwa_pe_finish_cached as bwa_cal_pac_pos_pe / bwa_paired_sw / bwa_refine_gapped do it (bwape.c:337-424,
 *                           635-658): a pair with both ends mapped and either end over popt->max_occ hits gets no multi-hit lists
 *                           (the `continue` at bwape.c:366); mate rescue runs only when popt->is_sw and ii->avg >= 0 (the -s / -A
 *                           switches and a chunk without an estimate).  *cnt_chg (may be NULL): the sum of pairing()'s returns.
 *                           The caller applies force_isize (-A) to *ii itself, as bwape.c:343-346 does.
 * nabwa_index_pac2real    = bns_coor_pac2real (bntseq.c:272-306): the contig of pac position pos and the number of ambiguous
 *                           bases under [pos, pos + len); needs nabwa_index_attach_reference. */
#define NABWA_ISIZE_FEW   1
#define NABWA_ISIZE_WEIRD 2
int nabwa_isize_infer_pairs(int n_pairs, const uint32_t *pos, const int32_t *len, const int32_t *mapq, double ap_prior, int64_t L,
							nabwa_isize_t *out, char *log, int log_cap);
int nabwa_pe_finish_sampe(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const nabwa_isize_t *ii,
						  int n_pairs, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, const int32_t *n_aln,
						  const nabwa_aln1_t *aln, nabwa_pe_t *inout, nabwa_poscache_t *cache, int *cnt_chg, uint64_t n_tot[2],
						  uint64_t n_mapped[2]);
int nabwa_index_pac2real(const nabwa_index_t *ix, int64_t pos, int len, int *seqid);

/* ---- colour space (SOLiD): `bwa samse` / `bwa sampe` on a .sai whose gap_opt_t.mode lacks BWA_MODE_COMPREAD ---------------------------
 * The reference refines the colour hits on the colour pac, turns every mapped colour read into a nucleotide read with nucleotide
 * qualities (bwa_cs2nt_core, cs2nt.c:112-191), refines every CIGAR again on the nucleotide pac and takes MD / NM from there
 * (bwa_refine_gapped with ntbns, bwase.c:356-423; no bwa_correct_trimmed).  The decoding is a per-read dynamic programme and runs on
 * the GPU, one read per lane.
 * nabwa_cs2nt                    = cs2nt_DP + cs2nt_nt_qual (cs2nt.c:36-109) for n cases: case i has size = off[i + 1] - off[i] colours
 *                                  (1 .. NABWA_CS2NT_MAX; off[0] = 0), cs_read[off[i] ..) = colour << 6 | quality (63: an N colour),
 *                                  nt_ref[off[i] + i ..) = size + 1 codes 0-4, and gets out[off[i] - i ..) = size - 1 bytes base << 6 | quality
 *                                  (0 where a neighbouring colour was N), the reference's returned array.
 * nabwa_index_attach_nt_reference = bwa_open_nt + bwt_restore_pac (bwase.c:595-603): <prefix>.nt.ann, .nt.amb and .nt.pac of an index built
 *                                  with `-c`; the 2-bit bases go to HBM.  After nabwa_index_attach_reference: coordinates, contig names
 *                                  and ambiguity holes stay those of the colour annotations, as in the reference.
 * nabwa_se_finish_cs             = nabwa_se_finish for colour reads.  qual: the reads' qualities as in the FASTQ (+33), read order, read i
 *                                  at off[i] (its first len characters).  Out, caller-owned and off[n] bytes each, read i at off[i]: nt_seq
 *                                  (the decoded read reversed, as bwa_seq_t.seq is held here), nt_rseq (its reverse complement), nt_qual
 *                                  (qualities + 33, read order); valid for mapped records, whose len and full_len become the decoded
 *                                  length (one less than the colours the alignment consumes); the other bytes come back 0.  Unmapped records keep the colour read.
 * nabwa_pe_finish_sampe_cs       = nabwa_pe_finish_sampe for colour pairs, the same side arrays (index 2 * pair + end).  popt->type must be 2
 *                                  (BWA_PET_SOLID: both ends on the fragment's strand, end 0 upstream, bwape.c:234-247), and popt->is_sw
 *                                  0 or ii->avg < 0: the reference's mate rescue dereferences a null pac in colour space (bwape.c:651,
 *                                  692-701), so there is nothing to reproduce.
 * Both return NABWA_EINVAL when opt->mode has COMPREAD set or the index has no nucleotide reference attached.
 * times (both chains, may be NULL): [0] += wall seconds of the decode stage (records, copies, kernels), [1] += HIP-event milliseconds
 *                                  of its kernels; added to, so that a caller sums over its chunks.
 * nabwa_pairing_typed            = nabwa_pairing with pe_opt_t.type (1 or 2). */
#define NABWA_CS2NT_MAX 1024
int nabwa_cs2nt(int device, int n, const int64_t *off, const uint8_t *nt_ref, const uint8_t *cs_read, uint8_t *out);
int nabwa_index_attach_nt_reference(nabwa_index_t *ix, const char *prefix);
int nabwa_se_finish_cs(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off, const uint8_t *seq, const uint8_t *rseq,
					   const uint8_t *qual, const int32_t *full_len, const int32_t *n_aln, const nabwa_aln1_t *aln, int n_occ,
					   uint64_t *rng48, nabwa_se_t *out, uint8_t *nt_seq, uint8_t *nt_rseq, uint8_t *nt_qual, double *times);
int nabwa_pe_finish_sampe_cs(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, const nabwa_pe_opt_t *popt, const nabwa_isize_t *ii,
							 int n_pairs, const int64_t *off, const uint8_t *seq, const uint8_t *rseq, const uint8_t *qual,
							 const int32_t *n_aln, const nabwa_aln1_t *aln, nabwa_pe_t *inout, nabwa_poscache_t *cache, int *cnt_chg,
							 uint8_t *nt_seq, uint8_t *nt_rseq, uint8_t *nt_qual, double *times);
int nabwa_pairing_typed(nabwa_pe_end_t p[2], int n_hits, uint64_t *hits, const nabwa_aln1_t *rows0, const nabwa_aln1_t *rows1,
						int max_isize, int s_mm, const nabwa_isize_t *ii, int type);

/* ---- BGZF on the GPU (bgzf_deflate.hip, nabwa_bgzf.hip): bytes in, BGZF blocks out.  Every block is a gzip member with the BC extra
 * field, its payload a valid RFC 1951 stream (fixed Huffman codes, or one stored block where that is shorter), CRC-32 and ISIZE made on
 * the device.  Only the INFLATED bytes are contract: the compressed bytes differ from zlib's and may change between versions.
 * nabwa_bgzf_bound            upper bound of the output for n input bytes (blocks of <= 0xff00 bytes, each <= 0x10000)
 * nabwa_bgzf_compress         n bytes -> ceil(n / 0xff00) BGZF blocks, back to back, WITHOUT the end-of-file block; n = 0 -> no block.
 *                             NABWA_ECAP with *n_out = needed if cap is too small, NABWA_ENODEV without a device.  No block is larger
 *                             than its slice + 31 bytes.
 * nabwa_bgzf_create / _handle_compress / _destroy: the same with a handle that keeps its stream, its device buffers and its pinned
 *                             staging buffers between calls (they grow to 1024 slices at most; longer inputs go through in chunks).
 *                             One call at a time per handle.
 * nabwa_bgzf_compress_ex / nabwa_bgzf_handle_compress_ex: the same with the codes to write; the two entries above are these with
 *                             NABWA_BGZF_CODES_FIXED and give the bytes they always gave.  NABWA_BGZF_CODES_DYNAMIC: the slices and their
 *                             tokens are the same, and a block may be stored, fixed or dynamic (BTYPE 10: codes of at most 15 bits built
 *                             from the slice's own histogram on the device).  It is dynamic where that is strictly shorter and the fixed
 *                             mode's block byte for byte where not, so no block is larger than the fixed mode's of the same slice, and
 *                             nabwa_bgzf_bound and the slice + 31 bytes hold.  Any other value of codes is NABWA_EINVAL.
 *
 * The inverse (bgzf_inflate.hip): whole BGZF members back to back in, their inflated bytes out.  Any RFC 1951 payload is read (stored,
 * fixed and dynamic blocks, several per member), not only what the compressor above writes; every member's length and CRC-32 are checked
 * against its trailer on the device.
 * nabwa_bgzf_inflated_size    host only, no device: walks the members' headers; the sum of ISIZE and the number of members (an empty
 *                             end-of-file block is a member).  NABWA_EDATA for a header that is not BGZF, a BSIZE that points past n, a
 *                             trailing partial member, or an ISIZE above 0x10000.
 * nabwa_bgzf_decompress       NABWA_ECAP with *n_out = needed if cap is too small (decided on the host before anything is launched),
 *                             NABWA_ENODEV without a device, NABWA_EDATA for what nabwa_bgzf_inflated_size refuses and for a member that
 *                             does not inflate to what its trailer says: nabwa_last_error names the member's index, its byte offset and
 *                             the reason.  On any error `out` may hold partial bytes.
 * nabwa_bgzf_handle_decompress the same on a handle of nabwa_bgzf_create (device buffers that grow and stay; inputs that inflate to more
 *                             than 256 MB go through in rounds of whole members).  One call at a time per handle, compress or decompress. */
typedef struct nabwa_bgzf nabwa_bgzf_t;
int nabwa_bgzf_inflated_size(const uint8_t *in, int64_t n, int64_t *n_out, int64_t *n_blocks);
int nabwa_bgzf_decompress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks);
int nabwa_bgzf_handle_decompress(nabwa_bgzf_t *z, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks);
int64_t nabwa_bgzf_bound(int64_t n);
int nabwa_bgzf_compress(int device, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks);
int nabwa_bgzf_create(int device, nabwa_bgzf_t **out);
int nabwa_bgzf_handle_compress(nabwa_bgzf_t *z, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks);
void nabwa_bgzf_destroy(nabwa_bgzf_t *z);
#define NABWA_BGZF_CODES_FIXED    0
#define NABWA_BGZF_CODES_DYNAMIC  1
int nabwa_bgzf_compress_ex(int device, int codes, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks);
int nabwa_bgzf_handle_compress_ex(nabwa_bgzf_t *z, int codes, const uint8_t *in, int64_t n, uint8_t *out, int64_t cap, int64_t *n_out, int64_t *n_blocks);

/* ---- coordinate sort of finished BAM records on the GPU (bam_sort.hip, bam_sort_body.hpp, rec_stream.hpp).  Record i is
 * in[in_off[i] .. in_off[i + 1]) as it stands in an uncompressed BAM stream: u32 block_size, then the block (refID at byte 4 and pos at
 * byte 8 of the record, little-endian int32); the offsets are those nabwa_bam_batch_output writes.  `out` receives the same records in
 * non-decreasing key order, records of equal key in the order they had in `in` (the sort is stable); out_off (n_rec + 1, may be NULL)
 * their offsets from 0 and keys_out (n_rec, may be NULL) their keys, both in output order.
 * The key of a record: the reference id as an unsigned word (so -1, unmapped without a place, sorts last), then pos + 1 (so -1 sorts first).
 * NABWA_EINVAL  a null argument; n_rec < 0 or above 0x7fffffff; offsets that do not increase; a record shorter than 36 bytes -- all decided
 *               on the host from the offsets alone, before the device is looked for (nabwa_bam_sort) and without touching the bytes
 * NABWA_ECAP    cap is below the records' total, in_off[n_rec] - in_off[0] (nabwa_last_error says how much is needed)
 * NABWA_EDATA   a record's block_size disagrees with its offsets (found on the device while the key is read); nabwa_last_error names the
 *               lowest such record.  `out` is not written
 * NABWA_ENODEV  no device;  NABWA_ENOMEM  the run does not fit the device: it needs 2 x the bytes + 40 B per record + the radix sort's
 *               scratch, and the caller picks the run size
 * n_rec == 0 is NABWA_OK with nothing written.  Nothing outside [out, out + cap) is written in any case.  There is no CPU path here.
 * nabwa_bam_sort_create / _run / _destroy: a handle that keeps its stream and its device buffers (they grow and stay) between calls, one call
 * at a time; nabwa_bam_sort is the handle used once.  nabwa_bam_sort_times: the device-event times of the handle's last successful run in
 * milliseconds -- upload, key kernel, radix sort, sizes + scan, gather kernel, download. */
#define NABWA_BAM_SORT_KEY(tid, pos) (((uint64_t)(uint32_t)(tid) << 32) | (uint32_t)((pos) + 1))
typedef struct nabwa_bam_sort nabwa_bam_sort_t;
int nabwa_bam_sort_create(int device, nabwa_bam_sort_t **out);
void nabwa_bam_sort_destroy(nabwa_bam_sort_t *s);
int nabwa_bam_sort_run(nabwa_bam_sort_t *s, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out);
int nabwa_bam_sort(int device, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out);
int nabwa_bam_sort_times(const nabwa_bam_sort_t *s, float ms[6]);

/* ---- damage profile of finished BAM records on the GPU (nabwa_damage.hip, damage_kernels.hip, damage_body.hpp, rec_stream.hpp, rec_body.hpp): the
 * substitutions of the mapped reads against the reference by distance from the read's ends, and the read lengths.  Records and offsets are
 * those of nabwa_bam_sort.  A record falls into the first class that fits, each with its counter in stats[]:
 *   skipped_flags  flag & exclude_flags, or (flag & require_flags) != require_flags
 *   skipped_place  refID < 0, refID >= the index's contigs, or pos < 0
 *   skipped_mapq   mapq < min_mapq
 *   skipped_empty  l_seq == 0 or n_cigar_op == 0
 *   counted        the CIGAR is walked from rp = contig[refID].offset + pos: M, = and X consume read and reference, I and S the read, D and
 *                  N the reference, H, P and the unassigned codes nothing.  A column of M / = / X with read index qi (0-based in the
 *                  stored seq, L = l_seq) and reference position k: a 4-bit read code other than A, C, G, T skips it
 *                  (columns_skipped_read); else k >= l_pac or k in a hole of the .amb skips it (columns_skipped_ref); else with the codes
 *                  A C G T = 0 1 2 3, forward strand (r, q, d5, d3) = (ref, read, qi, L - 1 - qi), flag 0x10 (3 - ref, 3 - read, L - 1 -
 *                  qi, qi) -- the substitution on the read's own strand, whose 5' end is the last stored base -- one is added to
 *                  sub5[min(d5, n_pos)][r][q] and to sub3[min(d3, n_pos)][r][q] (row n_pos: everything further in, the baseline; a column
 *                  of a short read counts near both ends) and to columns_counted; one to len_hist[min(L, NABWA_DAMAGE_LEN_BINS - 1)].
 *                  A record that runs over a contig's end is counted against the concatenated reference, as the reference's MD is.
 * NABWA_EINVAL  a null handle, index or option block; n_pos outside 1..256, which_ref outside 0..1; an index with no attached reference (no
 *               nucleotide reference when which_ref is 1); n_rec < 0 or above 0x7fffffff; offsets that do not increase; a record shorter
 *               than 36 bytes -- decided on the host from the arguments alone, the options before the index is looked at, everything
 *               before the device is
 * NABWA_EDATA   a block_size + 4 that is not the record's extent; 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq beyond the
 *               record, counted or skipped; a counted record whose CIGAR does not consume l_seq read bases.  nabwa_last_error names the
 *               lowest such record, and the failed call adds nothing to the handle's totals
 * NABWA_ENODEV  no device;  NABWA_ENOMEM  the call's records (their bytes + 8 per record) do not fit the device: the caller picks the size
 * n_rec == 0 is NABWA_OK.  There is no CPU path here.  No byte outside a record and no .pac byte at or past l_pac / 4 + 1 is read.
 * The handle works on the index's device with the index's copy of the reference (that of NABWA_FINISH=gpu: no second one), keeps its
 * stream and its device buffers (they grow and stay) between calls, one call at a time; THE INDEX MUST OUTLIVE THE HANDLE.
 * nabwa_damage_fetch: the totals of the successful calls since create / clear -- sub5 and sub3 (n_pos + 1) * 16 words each, index (p * 4 +
 * r) * 4 + q; len_hist NABWA_DAMAGE_LEN_BINS words; stats NABWA_DAMAGE_N_STATS words; any pointer may be NULL.  The counts are integer
 * sums: the same records give the same tables bit for bit, in any order and any split into calls.
 * nabwa_damage_times: device-event milliseconds of the last successful add -- upload, kernel, adding the call's table to the totals. */
#define NABWA_DAMAGE_LEN_BINS 1024
#define NABWA_DAMAGE_MAX_POS  256
enum { NABWA_DAMAGE_STAT_SEEN = 0, NABWA_DAMAGE_STAT_COUNTED, NABWA_DAMAGE_STAT_SKIPPED_FLAGS, NABWA_DAMAGE_STAT_SKIPPED_PLACE,
	   NABWA_DAMAGE_STAT_SKIPPED_MAPQ, NABWA_DAMAGE_STAT_SKIPPED_EMPTY, NABWA_DAMAGE_STAT_COLUMNS_COUNTED,
	   NABWA_DAMAGE_STAT_COLUMNS_SKIPPED_READ, NABWA_DAMAGE_STAT_COLUMNS_SKIPPED_REF, NABWA_DAMAGE_N_STATS };
typedef struct { int32_t n_pos; int32_t min_mapq; uint32_t exclude_flags; uint32_t require_flags; int32_t which_ref; int32_t pad; } nabwa_damage_opt_t;
typedef struct nabwa_damage nabwa_damage_t;
void nabwa_damage_default_opt(nabwa_damage_opt_t *o);      /* n_pos 25, min_mapq 0, exclude_flags 0xF04 (unmapped, secondary, QC-fail, duplicate, supplementary), require_flags 0, which_ref 0 */
int nabwa_damage_create(nabwa_index_t *ix, const nabwa_damage_opt_t *opt, nabwa_damage_t **out);
int nabwa_damage_add(nabwa_damage_t *d, int64_t n_rec, const uint8_t *in, const int64_t *in_off);
int nabwa_damage_fetch(nabwa_damage_t *d, uint64_t *sub5, uint64_t *sub3, uint64_t *len_hist, uint64_t *stats);
int nabwa_damage_clear(nabwa_damage_t *d);
void nabwa_damage_destroy(nabwa_damage_t *d);
int nabwa_damage_times(const nabwa_damage_t *d, float ms[3]);

/* ---- the coordinate sort once more, with the permutation: perm_out (n_rec, may be NULL) receives for each output record the index it had
 * in `in`.  The sort carries this index on the device anyway, so it is one more download.  nabwa_bam_sort_run and nabwa_bam_sort are these
 * with NULL. */
int nabwa_bam_sort_run_ex(nabwa_bam_sort_t *s, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out);
int nabwa_bam_sort_ex(int device, int64_t n_rec, const uint8_t *in, const int64_t *in_off, uint8_t *out, int64_t cap, int64_t *out_off, uint64_t *keys_out, uint32_t *perm_out);

/* ---- duplicate marking of finished BAM records on the GPU (nabwa_markdup.hip, markdup_kernels.hip, markdup_body.hpp, rec_stream.hpp, rec_body.hpp).
 * Records and offsets are those of nabwa_bam_sort.  The records get ordinals 0, 1, ... in the order they are added to a handle, across
 * calls; at most 0x7fffffff between create / clear.  A record falls into the first class that fits, each with its counter in stats[]:
 *   skipped_flags  flag & exclude_flags: never marked, in no group
 *   already        flag & 0x400: in no group, reported dup = 0 (the caller's flag stands)
 *   unmapped       flag & 0x4, refID < 0, pos < 0 or n_cigar_op == 0: in no group (but see "half pair")
 *   pair           records i and i + 1 of one call are mates when i has flags 0x1 and 0x40 (and not 0x80), i + 1 has 0x1 and 0x80 (and not
 *                  0x40), their read names are equal (length and bytes) and neither is skipped_flags or already.  Both mates mapped: a
 *                  pair (stats[pairs] counts it once).  Exactly one mapped, a half pair: the mapped mate is a fragment, the unmapped mate
 *                  (counted in unmapped) takes whatever mark its mate gets.  MATES MUST COME IN ONE CALL, next to each other
 *   fragment       every other mapped record; one with flag 0x1 that has no mate next to it also counts in orphans
 * Ends.  With the CIGAR's M, D, N, = and X consuming the reference, `lead` the S and H lengths before the first such operation (all of them
 * if there is none) and `trail` those after the last (0 if there is none): left = pos - lead, right = pos + (the reference consumed) - 1 +
 * trail, in 64 bits.  The 5' end of a record is (refID, strand, c5) with c5 = left on the forward strand and right with flag 0x10; c3 is
 * the other of the two.  Score: the sum of the base qualities >= min_qual, 0xff counting as 0; of a pair the sum over both mates; capped at
 * 0xfffffffe.
 * Groups.  Fragments are equal on (refID, strand, c5), with single_ends = NABWA_MARKDUP_ENDS_BOTH on (refID, strand, c5, c3) (collapsed or
 * merged reads, whose two ends are both real).  Pairs are equal on their two ends, the lower end first.  With NABWA_MARKDUP_ENDS_5P every
 * pair also stands in the fragment groups of its two ends as a shadow that outranks every fragment and is never itself marked: a fragment
 * that starts where a pair's mate starts is a duplicate (the rule of Picard and samtools).  ENDS_BOTH makes no shadows.
 * Winner.  Within a group the highest score wins, then the lowest ordinal; every other real member gets dup = 1, of a pair both mates.  The
 * result depends on nothing else: not on how the records were split into calls (mates together) and not on the device.
 * NABWA_EINVAL  a null argument; min_qual outside 0..255, single_ends outside 0..1; n_rec < 0 or above 0x7fffffff, or more than 0x7fffffff
 *               records in the handle; offsets that do not increase; a record shorter than 36 bytes -- decided on the host from the
 *               arguments alone, before the device is touched
 * NABWA_ECAP    nabwa_markdup_resolve: cap is below the records added
 * NABWA_EDATA   a block_size + 4 that is not the record's extent; 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq beyond the
 *               record, whatever its class; a mapped record with l_seq > 0 whose CIGAR does not consume l_seq read bases; a mapped record
 *               with left < -2^30 or right >= 2^31 + 2^30.  nabwa_last_error names the lowest such record, and the failed call adds nothing
 * NABWA_ENODEV  no device;  NABWA_ENOMEM  the device cannot hold it: a call needs its bytes + 28 B per record, the handle keeps 1 B per
 *               record and 24 B per tuple (a fragment is one tuple, a pair three, without shadows one), a resolve needs 25 B per tuple more
 * n_rec == 0 and a resolve with nothing added are NABWA_OK.  There is no CPU path here.  No byte outside the call's records is read.
 * nabwa_markdup_resolve: dup[ordinal] (0 or 1) and stats (NABWA_MARKDUP_N_STATS words, may be NULL) for everything added since create /
 * clear; it may be called again after more adds.  dup_fragments and dup_pairs count marked tuples, dup_records the records with dup = 1.
 * The handle keeps its stream, its arena and its scratch (they grow and stay) between calls, one call at a time.
 * nabwa_markdup_times: device-event milliseconds -- of the last successful add: upload, signature and tuple kernels; of the last resolve:
 * radix sorts, mark kernels, download. */
#define NABWA_MARKDUP_ENDS_5P   0
#define NABWA_MARKDUP_ENDS_BOTH 1
enum { NABWA_MARKDUP_STAT_SEEN = 0, NABWA_MARKDUP_STAT_SKIPPED_FLAGS, NABWA_MARKDUP_STAT_ALREADY, NABWA_MARKDUP_STAT_UNMAPPED,
	   NABWA_MARKDUP_STAT_FRAGMENTS, NABWA_MARKDUP_STAT_PAIRS, NABWA_MARKDUP_STAT_ORPHANS, NABWA_MARKDUP_STAT_DUP_FRAGMENTS,
	   NABWA_MARKDUP_STAT_DUP_PAIRS, NABWA_MARKDUP_STAT_DUP_RECORDS, NABWA_MARKDUP_N_STATS };
typedef struct { int32_t min_qual; int32_t single_ends; uint32_t exclude_flags; int32_t pad; } nabwa_markdup_opt_t;
typedef struct nabwa_markdup nabwa_markdup_t;
void nabwa_markdup_default_opt(nabwa_markdup_opt_t *o);    /* min_qual 15, NABWA_MARKDUP_ENDS_5P, exclude_flags 0xB00 (secondary, QC-fail, supplementary) */
int nabwa_markdup_create(int device, const nabwa_markdup_opt_t *opt, nabwa_markdup_t **out);
int nabwa_markdup_add(nabwa_markdup_t *m, int64_t n_rec, const uint8_t *in, const int64_t *in_off);
int nabwa_markdup_resolve(nabwa_markdup_t *m, uint8_t *dup, int64_t cap, uint64_t *stats);
int nabwa_markdup_clear(nabwa_markdup_t *m);
void nabwa_markdup_destroy(nabwa_markdup_t *m);
int nabwa_markdup_times(const nabwa_markdup_t *m, float ms[5]);

/* ---- the BAM index (.bai, SAM specification 5.2) of finished, coordinate-sorted BAM records on the GPU (nabwa_bai.hip, bai_kernels.hip,
 * bai_body.hpp, rec_stream.hpp, rec_body.hpp).  Records and offsets are those of nabwa_bam_sort; n_ref is the number of reference sequences of the header.
 * nabwa_bai_add takes records in the order of the file.  stream_off is where in[in_off[0]] lies in the uncompressed BAM stream, the header
 * included; it is not below the end of the records added before (gaps are allowed).
 * A record.  tid, pos and flag are its fields; end = pos + the lengths of its M, D, N, = and X operations, or pos + 1 with flag 0x4, without
 * a CIGAR or where that sum is 0; beg = pos; bin = reg2bin(beg, end) of the specification (the record's own bin field is not read).  A
 * record with tid < 0 has no place: it is only counted (n_no_coor).
 * nabwa_bai_finish takes the BGZF blocks of the finished file: blk_uoff[b] and blk_coff[b] are where block b starts in the uncompressed
 * stream and in the file, entry n_blk being the end-of-file block (blk_uoff[n_blk] is the stream's length).  The virtual offset of stream
 * offset U is blk_coff[b] << 16 | (U - blk_uoff[b]) with b the last block that has blk_uoff[b] <= U; the stream's end is therefore the
 * end-of-file block at 0.
 * The file, fully determined: "BAI\1", n_ref; per reference its bins in rising number, only those that hold records; within a bin the
 * records in stream order, a record starting a new chunk unless its start lies in the BGZF block in which the bin's previous record ends
 * (vend >> 16 == vbeg >> 16), a chunk running from its first record's start to its last record's end; a reference with records has
 * pseudo-bin 37450 last, with the chunks (start of its first record, end of its last) and (records without flag 0x4, records with it);
 * the linear index has 1 + max((end - 1) >> 14) windows, windows beg >> 14 .. (end - 1) >> 14 of a record taking the lowest start of the
 * records that touch them, an untouched window the next touched one's value; a reference without records has n_bin = 0 and n_intv = 0;
 * the file ends with the 64-bit count of the records with tid < 0.
 * NABWA_EINVAL  a null argument; n_ref < 0; n_rec, offsets and record sizes as nabwa_markdup_add; a stream_off below 0 or below the end of
 *               the last add; nabwa_bai_finish: n_blk < 0, a blk_uoff that falls, a blk_coff that does not rise, a block of more than 65536
 *               bytes, a blk_coff of 2^48 or more, a record added that starts before blk_uoff[0] or ends behind blk_uoff[n_blk], more than
 *               0x7fffffff windows -- decided on the host, before the device is touched
 * NABWA_ECAP    nabwa_bai_finish: cap is below the file's size (*n_out says it)
 * NABWA_EDATA   a block_size + 4 that is not the record's extent; 36 + l_read_name + 4 n_cigar_op + (l_seq + 1) / 2 + l_seq beyond the
 *               record; tid >= n_ref; tid >= 0 with pos < 0; end > 2^29; a NABWA_BAM_SORT_KEY below that of the record in front of it, the
 *               last record of the add before included.  nabwa_last_error names the lowest such record, and the failed call adds nothing
 * NABWA_ENODEV  no device;  NABWA_ENOMEM  the device cannot hold it: a call needs its bytes + 8 B per record, the handle keeps 32 B per
 *               record, a finish needs 60 B per record more, 8 B per window and the file
 * n_rec == 0 and a finish with nothing added are NABWA_OK.  There is no CPU path here.  No byte outside the call's records is read.
 * nabwa_bai_finish with out == NULL (cap 0) only says the size in *n_out.  It does not consume the handle: more adds and another finish
 * may follow.  stats (NABWA_BAI_N_STATS words, may be NULL): the records added, those with a place, those without, the bins and the chunks
 * written (pseudo-bins not counted), the windows, the file's bytes.
 * nabwa_bai_times: device-event milliseconds -- of the last successful add: upload, signature kernel; of the last finish that wrote a
 * file: radix sort, virtual offsets / chunks / layout, linear index, writer kernels, download. */
enum { NABWA_BAI_STAT_RECORDS = 0, NABWA_BAI_STAT_PLACED, NABWA_BAI_STAT_NO_COOR, NABWA_BAI_STAT_BINS, NABWA_BAI_STAT_CHUNKS, NABWA_BAI_STAT_WINDOWS,
	   NABWA_BAI_STAT_BYTES, NABWA_BAI_N_STATS };
typedef struct nabwa_bai nabwa_bai_t;
int nabwa_bai_create(int device, int32_t n_ref, nabwa_bai_t **out);
int nabwa_bai_add(nabwa_bai_t *b, int64_t n_rec, const uint8_t *in, const int64_t *in_off, int64_t stream_off);
int nabwa_bai_finish(nabwa_bai_t *b, int64_t n_blk, const int64_t *blk_uoff, const int64_t *blk_coff, uint8_t *out, int64_t cap, int64_t *n_out, uint64_t *stats);
int nabwa_bai_clear(nabwa_bai_t *b);
void nabwa_bai_destroy(nabwa_bai_t *b);
int nabwa_bai_times(const nabwa_bai_t *b, float ms[7]);
/* host only, no device: the block table of whole BGZF members back to back, for nabwa_bai_finish, from their BSIZE and ISIZE fields.  The
 * last member is taken as the end-of-file block: *n_blk is the number of members before it, and both arrays (either may be NULL) take
 * *n_blk + 1 entries where cap (in entries) allows; NABWA_ECAP where it does not (*n_blk is set), NABWA_EDATA for what
 * nabwa_bgzf_inflated_size refuses, for no member at all and for a last member that is not empty */
int nabwa_bgzf_block_table(const uint8_t *in, int64_t n, int64_t *blk_uoff, int64_t *blk_coff, int64_t cap, int64_t *n_blk);

#ifdef __cplusplus
}
#endif
#endif
