// rec_body.hpp -- what the bodies of the record-stream modules share (markdup_body.hpp, bai_body.hpp, damage_body.hpp; bam_sort_body.hpp takes
// the two constants): a call's input is n_rec finished BAM records as bytes and off[n_rec + 1], and a persistent grid of
// workgroups of REC_BLOCK threads takes them REC_GROUPS per trip, REC_LANES lanes per record.
//
//   REC_FN, REC_HD, REC_THREADS, REC_SYNC, REC_ADD32 ... rec_fetch_add    the one layer between the bodies and where they run
//   rec_u32, rec_op_read, rec_op_ref    a word at any byte address; what a CIGAR operation consumes
//   REC_FIELDS, REC_NEED, REC_HEAD      the fixed fields of a record, the bytes they ask for, and the two kinds of damage every module looks for
//
// Compiled for gfx950 by the modules' kernel files and, with NABWA_EMU (tests/emu/, test infrastructure), by g++: there the threads of a
// workgroup run one after the other between the barriers, so that every address the bodies form can be checked under AddressSanitizer
// without a GPU.
#pragma once
#include <stdint.h>
#ifdef NABWA_EMU
#define REC_FN static inline
#define REC_HD static inline
#define REC_THREADS for (int tid = 0; tid < REC_BLOCK; ++tid)
#define REC_SYNC ((void)0)
#define REC_INC(p) (++*(p))
#define REC_ADD32(p, v) (*(p) += (v))
#define REC_ADD64(p, v) (*(p) += (v))
#define REC_OR(p, v) (*(p) |= (v))
#define REC_MIN32(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
#define REC_MAX32(p, v) (*(p) = *(p) > (v) ? *(p) : (v))
#define REC_MIN64(p, v) (*(p) = *(p) < (v) ? *(p) : (v))
static inline unsigned int rec_fetch_add(unsigned int *p, unsigned int v) { const unsigned int o = *p; *p = o + v; return o; }
#else
#define REC_FN __device__ __forceinline__
#define REC_HD __host__ __device__ __forceinline__
#define REC_THREADS for (int tid = (int)threadIdx.x, once_ = 1; once_; once_ = 0)
#define REC_SYNC __syncthreads()
#define REC_INC(p) ((void)atomicAdd((p), 1u))
#define REC_ADD32(p, v) ((void)atomicAdd((p), (v)))
#define REC_ADD64(p, v) ((void)atomicAdd((p), (v)))
#define REC_OR(p, v) ((void)atomicOr((p), (v)))
#define REC_MIN32(p, v) ((void)atomicMin((p), (v)))
#define REC_MAX32(p, v) ((void)atomicMax((p), (v)))
#define REC_MIN64(p, v) ((void)atomicMin((p), (v)))
#define rec_fetch_add(p, v) atomicAdd((p), (v))
#endif

#define REC_LANES   16                          /* lanes per record */
#define REC_BLOCK   256
#define REC_GROUPS  (REC_BLOCK / REC_LANES)     /* records per workgroup and trip */
#define REC_MIN_REC 36                          /* block_size + the 32 fixed bytes of a record */

/* a record starts at any byte, so nothing in it is aligned; the hardware reads a global word at any byte address */
REC_HD uint32_t rec_u32(const uint8_t *p) { uint32_t v; __builtin_memcpy(&v, p, 4); return v; }
REC_HD bool rec_op_read(uint32_t op) { return op == 0 || op == 1 || op == 4 || op == 7 || op == 8; }     /* M I S = X */
REC_HD bool rec_op_ref(uint32_t op) { return op == 0 || op == 2 || op == 3 || op == 7 || op == 8; }      /* M D N = X */

/* The fixed fields behind block_size of the record at `rec`, of at least REC_MIN_REC bytes, as constants of the block that names this;
 * nothing is checked.  L is l_seq.  (Macros, where the rest of this file is functions: a function that fills a struct, and one that returns
 * false for damage, leave the compiler a join in front of each body that it does not take apart again, and the kernels came out with other
 * registers -- the damage kernel with two more.  As text, each body compiles to what it was.) */
#define REC_FIELDS(rec) \
	const int32_t ref_id = (int32_t)rec_u32((rec) + 4), pos = (int32_t)rec_u32((rec) + 8); \
	const uint32_t w12_ = rec_u32((rec) + 12), w16_ = rec_u32((rec) + 16); \
	const uint32_t l_name = w12_ & 0xffu, mapq = w12_ >> 8 & 0xffu, n_cig = w16_ & 0xffffu, flag = w16_ >> 16; \
	const uint64_t L = rec_u32((rec) + 20); \
	(void)ref_id; (void)pos; (void)l_name; (void)mapq; (void)n_cig; (void)flag; (void)L
/* the bytes that a record's name, CIGAR, bases and qualities ask for, the fixed ones included */
#define REC_NEED(l_name, n_cig, L) ((uint64_t)REC_MIN_REC + (l_name) + 4 * (uint64_t)(n_cig) + ((L) + 1) / 2 + (L))
/* how a *_record_part starts: the fields of `rec` of `size` >= REC_MIN_REC bytes, and `return bad` for either damage that every module
 * looks for -- a block_size that is not what the offsets say (before any other field is read), variable parts that do not fit the record */
#define REC_HEAD(rec, size, bad) \
	if ((int64_t)rec_u32(rec) + 4 != (size)) return (bad); \
	REC_FIELDS(rec); \
	if (REC_NEED(l_name, n_cig, L) > (uint64_t)(size)) return (bad)
