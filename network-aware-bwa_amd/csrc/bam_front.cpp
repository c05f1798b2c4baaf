// bam_front.cpp -- the create stage of the BAM front-end: read_bam_pair (bwaseqio.c:340-494) and bam1_to_seq (bwaseqio.c:272-307) over a batch
// of records instead of one logical record at a time.  tests/emu/bam_front_main.cpp runs these stages on the CPU, against the reference's own
// functions (tests/golden/vectors_bam_front.npz) and under sanitizers.
#include <string.h>
#include <map>
#include <string>
#include <utility>
#include <vector>
#include "bam_front.hpp"

int bam_front_parse(nabwa_bam_batch *b, int n_rec, const uint8_t *in, const int64_t *in_off, uint32_t *any_flag)
{
	*any_flag = 0;
	if (!b->rec.make((size_t)n_rec)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the records");
	for (int i = 0; i < n_rec; ++i) if (in_off[i + 1] - in_off[i] < 36 || in_off[i + 1] - in_off[i] > (int64_t)1 << 28) return nabwa_fail(NABWA_EINVAL, "malformed BAM record");
	if (!b->arena.take((size_t)(n_rec ? in_off[n_rec] - in_off[0] : 0) + (size_t)n_rec * (REC_ROOM - 36) + 64)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the records");
	const int nt = host_threads((size_t)n_rec, BAM_MIN_N);
	std::vector<int> bad(nt, 0);
	std::vector<uint32_t> flag_or((size_t)nt * 16, 0u);          /* (a line per thread) */
	host_parallel(nt, (size_t)n_rec, [&](int t, size_t lo, size_t hi) {
		uint32_t fo = 0;
		for (size_t i = lo; i < hi; ++i) {
			/* one pass over a record while it is in the cache: parse, erase_unwanted_tags, bam_get_rg (neither depends on how the records
			 * pair up; a record the pairing drops has been cleaned in vain) */
			BamRec &r = b->rec[i];
			if (!parse_rec(in + in_off[i], in_off[i + 1] - in_off[i], r, b->arena.get() + (in_off[i] - in_off[0]) + i * (size_t)(REC_ROOM - 36))) { bad[t] = 1; continue; }
			if (!erase_tags(r)) { bad[t] = 2; continue; }
			const auto v = get_rg(r);
			r.rg_p = v.first; r.rg_n = (uint32_t)v.second;
			fo |= r.flag;
		}
		flag_or[(size_t)t * 16] = fo;
	});
	for (int x : bad) if (x) return nabwa_fail(NABWA_EINVAL, x == 2 ? "malformed tags in a BAM record" : "malformed BAM record");
	for (size_t t = 0; t < flag_or.size(); t += 16) *any_flag |= flag_or[t];
	return NABWA_OK;
}

/* read_bam_pair_core (bwaseqio.c:346-410) from record i on: 1 or 2 = the kind of the logical record that starts at i (mates swapped or
 * their flags mended where the reference does), 0 = record i is discarded (allow_broken), < 0 = an error that has been reported */
static int pair_at(nabwa_bam_batch *b, int i, bool broken)
{
	BamRec &r0 = b->rec[i];
	if (!(r0.flag & F_PD)) return 1;
	if (i + 1 >= (int)b->rec.size()) return broken ? 0 : nabwa_fail(NABWA_EINVAL, "a paired read at the end of the batch without its mate (keep mates in one batch)");
	BamRec &r1 = b->rec[i + 1];
	const uint32_t f0 = r0.flag & (F_PD | F_R1 | F_R2), f1 = r1.flag & (F_PD | F_R1 | F_R2);
	if (strcmp((const char*)r0.data.data(), (const char*)r1.data.data()) != 0)
		return broken ? 0 : nabwa_fail(NABWA_EINVAL, "lone mate: two paired reads whose names do not match");
	if (f0 == (F_PD | F_R2) && f1 == (F_PD | F_R1)) std::swap(r0, r1);
	else if (!(f0 == (F_PD | F_R1) && f1 == (F_PD | F_R2))) {
		if (!broken) return nabwa_fail(NABWA_EINVAL, "a pair whose read 1 / read 2 flags are wrong");
		r0.flag = (r0.flag & ~(uint32_t)F_R2) | F_PD | F_R1; r1.flag = (r1.flag & ~(uint32_t)F_R1) | F_PD | F_R2;
	}
	return 2;
}

/* Logical records (read_bam_pair_core, bwaseqio.c:346-410): a paired read takes the next record as its mate -- same name, flags read 1 /
 * read 2 in either order.  Anything else is an error, or with NABWA_BAM_BROKEN_INPUT (allow_broken) is mended as the reference mends it:
 * wrong flags are set right, a paired read whose successor has another name is discarded and that successor starts the next logical
 * record, a paired read with nothing after it is discarded.  NABWA_BAM_DROP_ALIGNED (read_bam_pair's ignore_aligned, bwaseqio.c:466-474)
 * leaves out logical records any read of which is already mapped.  src: the records that stay, in their new order. */
static int pair_general(nabwa_bam_batch *b, std::vector<int> &src)
{
	const bool broken = (b->flags & NABWA_BAM_BROKEN_INPUT) != 0, drop = (b->flags & NABWA_BAM_DROP_ALIGNED) != 0, nodup = (b->flags & NABWA_BAM_SKIP_DUPLICATES) != 0;
	const int n_rec = (int)b->rec.size();
	src.reserve(n_rec); b->kind.reserve(n_rec); b->first.reserve(n_rec); b->skip.reserve(n_rec);
	for (int i = 0; i < n_rec; ) {
		const int k = pair_at(b, i, broken);
		if (k < 0) return k;
		if (k == 0) { ++i; continue; }          /* (the last record of the batch, or a lone mate whose successor starts the next record) */
		BamRec &r0 = b->rec[i];
		const uint32_t all = r0.flag & (k == 2 ? b->rec[i + 1].flag : ~0u), any = r0.flag | (k == 2 ? b->rec[i + 1].flag : 0u);
		if (!(drop && !(all & F_SU))) {
			if (k == 2) { BamRec &r1 = b->rec[i + 1]; r0.flag |= r1.flag & F_QC; r1.flag |= r0.flag & F_QC; }          /* either none or both pass QC (bwaseqio.c:486-489) */
			b->kind.push_back(k); b->first.push_back((int)src.size()); b->skip.push_back(nodup && (any & F_DP));
			for (int e = 0; e < k; ++e) src.push_back(i + e);
		}
		i += k;
	}
	return NABWA_OK;
}

int bam_front_pair(nabwa_bam_batch *b, uint32_t any_flag)
{
	const size_t n_rec = b->rec.size();
	if (!(any_flag & F_PD) && !(b->flags & (NABWA_BAM_DROP_ALIGNED | NABWA_BAM_SKIP_DUPLICATES))) {
		/* single-end records only and nothing to leave out: every record is a logical record of its own */
		b->kind.assign(n_rec, 1); b->skip.assign(n_rec, 0); b->first.resize(n_rec);
		int *const fp = b->first.data();
		host_parallel(host_threads(n_rec, BAM_MIN_N), n_rec, [fp](int, size_t lo, size_t hi) { for (size_t i = lo; i < hi; ++i) fp[i] = (int)i; });
		return NABWA_OK;
	}
	std::vector<int> src;
	const int rc = pair_general(b, src);
	if (rc != NABWA_OK) return rc;
	if (src.size() != n_rec) {
		RecArr kept;
		if (!kept.make(src.size())) return nabwa_fail(NABWA_ENOMEM, "out of memory for the records");
		for (size_t t = 0; t < src.size(); ++t) kept[t] = std::move(b->rec[src[t]]);
		b->rec.swap(kept);
	}
	return NABWA_OK;
}

void bam_front_read_groups(nabwa_bam_batch *b)
{
	const size_t nk = b->kind.size();
	b->rg.resize(nk);
	std::map<std::string, int> ids;
	/* "the same read group as the logical record before" by all threads (the records' bytes are touched there); the names that change, in order, by one */
	std::vector<uint8_t> same_rg(nk ? nk : 1, 0);
	host_parallel(host_threads(nk, BAM_MIN_N), nk, [&](int, size_t lo, size_t hi) {
		for (size_t k = lo ? lo : 1; k < hi; ++k) {
			const BamRec &r0 = b->rec[b->first[k]], &rp = b->rec[b->first[k - 1]];
			same_rg[k] = r0.rg_n == rp.rg_n && !memcmp(r0.rg_p, rp.rg_p, r0.rg_n);
		}
	});
	for (size_t k = 0; k < nk; ++k) {
		if (same_rg[k]) { b->rg[k] = b->rg[k - 1]; continue; }
		const BamRec &r0 = b->rec[b->first[k]];
		auto ins = ids.emplace(std::string((const char*)r0.rg_p, r0.rg_n), (int)b->rg_names.size());
		if (ins.second) b->rg_names.push_back(ins.first->first);
		b->rg[k] = ins.first->second;
	}
}

/* the (trimmed) lengths first, then every thread encodes its slice of the reads in place */
int bam_front_encode(nabwa_bam_batch *b)
{
	const size_t n_rec = b->rec.size();
	const int trim_qual = b->opt.trim_qual;
	b->off.assign(n_rec + 1, 0); b->full_len.assign(n_rec ? n_rec : 1, 0);
	std::vector<int32_t> lens(n_rec ? n_rec : 1, 0);
	std::vector<uint8_t> rskip(n_rec ? n_rec : 1, 0);       /* a duplicate that is passed through is searched as a read without bases */
	for (size_t k = 0; k < b->kind.size(); ++k) if (b->skip[k]) for (int e = 0; e < b->kind[k]; ++e) rskip[b->first[k] + e] = 1;
	host_parallel(host_threads(n_rec, BAM_MIN_N), n_rec, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) { lens[i] = rskip[i] ? 0 : rec_trimmed_len(b->rec[i], trim_qual); b->full_len[i] = b->rec[i].l_qseq; }
	});
	for (size_t i = 0; i < n_rec; ++i) b->off[i + 1] = b->off[i] + lens[i];
	if (!b->seq.alloc((size_t)b->off[n_rec] + 1) || !b->rseq.alloc((size_t)b->off[n_rec] + 1)) return nabwa_fail(NABWA_ENOMEM, "out of memory for the reads");
	host_parallel(host_threads(n_rec, BAM_MIN_N), n_rec, [&](int, size_t lo, size_t hi) {
		for (size_t i = lo; i < hi; ++i) rec_encode(b->rec[i], lens[i], b->seq.data() + b->off[i], b->rseq.data() + b->off[i]);
	});
	b->seq.data()[b->off[n_rec]] = 0; b->rseq.data()[b->off[n_rec]] = 0;
	return NABWA_OK;
}
