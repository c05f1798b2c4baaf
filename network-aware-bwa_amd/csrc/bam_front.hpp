// bam_front.hpp -- what nabwa_bam_batch_create does with the caller's records, as stages over the new batch (bam_front.cpp).  Host only: no
// stage looks at the index.  Each returns NABWA_OK or what nabwa_fail returned; the batch is the caller's to destroy either way.
#pragma once
#include "bam_batch.hpp"

/* parse every record into the batch's arena, erase the tags the aligner makes anew and find the read group, by all threads; *any_flag: the
 * OR of the records' flags */
int bam_front_parse(nabwa_bam_batch *b, int n_rec, const uint8_t *in, const int64_t *in_off, uint32_t *any_flag);
/* singletons and pairs by read_bam_pair's rules under b->flags: kind, first, skip; records that are left out leave b->rec */
int bam_front_pair(nabwa_bam_batch *b, uint32_t any_flag);
/* rg and rg_names: the read group of every logical record, numbered in the order they are first seen */
void bam_front_read_groups(nabwa_bam_batch *b);
/* bam1_to_seq of every record under b->opt.trim_qual: off, full_len, seq, rseq */
int bam_front_encode(nabwa_bam_batch *b);
