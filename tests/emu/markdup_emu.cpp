// tests/emu/markdup_emu.cpp -- TEST INFRASTRUCTURE ONLY.  The bodies of duplicate marking (csrc/markdup_body.hpp) compiled by g++ and run on the
// CPU as nabwa_markdup.hip strings them together: the workgroups of the signature grid one after the other into the call's scratch, the tuples
// of a sound call onto the arena, and for a resolve three stable sorts of the tuple indexes by k3, lo and hi, the marks and the mates' marks.
// Every buffer is exactly as long as the bodies may use it, so that AddressSanitizer sees a byte too many.
#define NABWA_EMU 1
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <vector>
#include "../../network-aware-bwa_amd/csrc/markdup_body.hpp"

struct EmuMarkdup {
	int32_t min_qual, single_ends; uint32_t exclude_flags;
	std::vector<uint64_t> hi, lo, k3;
	std::vector<uint8_t> link;
	unsigned int n_tup = 0;
	unsigned long long stats[NABWA_MARKDUP_N_STATS] = {};
	int64_t n_ord = 0;
};

extern "C" void *emu_markdup_create(int min_qual, int single_ends, uint32_t exclude_flags)
{
	EmuMarkdup *m = new EmuMarkdup;
	m->min_qual = min_qual; m->single_ends = single_ends; m->exclude_flags = exclude_flags;
	return m;
}
extern "C" void emu_markdup_destroy(void *h) { delete (EmuMarkdup*)h; }
extern "C" void emu_markdup_clear(void *h)
{
	EmuMarkdup *m = (EmuMarkdup*)h;
	m->hi.clear(); m->lo.clear(); m->k3.clear(); m->link.clear(); m->n_tup = 0; m->n_ord = 0;
	memset(m->stats, 0, sizeof m->stats);
}

/* one call: -1 and the records added, or the lowest damaged record and the handle as it was.  n_blocks: the workgroups of the grid; reverse:
 * the tuples are appended from the last record to the first (the order of the arena is no one's to rely on).  No byte outside
 * in[off[0], off[n]) is read. */
extern "C" int64_t emu_markdup_add(void *h, int64_t n_rec, const uint8_t *in, const int64_t *off, int n_blocks, int reverse)
{
	EmuMarkdup *m = (EmuMarkdup*)h;
	if (n_rec == 0) return -1;
	std::vector<uint64_t> end((size_t)n_rec);
	std::vector<uint32_t> c3((size_t)n_rec), score((size_t)n_rec), meta((size_t)n_rec);
	MdParams P;
	P.in = in + off[0]; P.off = off; P.base = off[0]; P.n_rec = (int32_t)n_rec;
	P.min_qual = m->min_qual; P.single_ends = m->single_ends; P.exclude_flags = m->exclude_flags;
	P.end = end.data(); P.c3 = c3.data(); P.score = score.data(); P.meta = meta.data();
	unsigned int bad = 0xffffffffu;
	for (int b = 0; b < n_blocks; ++b) {
		unsigned long long sum[MD_GROUPS]; uint32_t diff[MD_GROUPS], lmeta[MD_GROUPS];
		memset(sum, 0xa5, sizeof sum); memset(diff, 0xa5, sizeof diff); memset(lmeta, 0xa5, sizeof lmeta);      /* (LDS starts out as anything) */
		md_block(P, sum, diff, lmeta, &bad, b, n_blocks);
		for (int g = 0; g < MD_GROUPS; ++g) if (sum[g] || diff[g]) return -2;      /* a workgroup leaves its words zero */
	}
	if (bad != 0xffffffffu) return (int64_t)bad;
	const size_t room = (size_t)m->n_tup + (size_t)((3 * n_rec + 1) / 2);
	m->hi.resize(room); m->lo.resize(room); m->k3.resize(room); m->link.resize((size_t)(m->n_ord + n_rec));
	MdArena A;
	A.hi = m->hi.data(); A.lo = m->lo.data(); A.k3 = m->k3.data(); A.link = m->link.data(); A.n_tup = &m->n_tup; A.stats = m->stats; A.ord_base = (uint32_t)m->n_ord;
	for (int64_t k = 0; k < n_rec; ++k) md_emit_record(P, A, reverse ? n_rec - 1 - k : k);
	if (m->n_tup > room) return -3;
	m->hi.resize(m->n_tup); m->lo.resize(m->n_tup); m->k3.resize(m->n_tup);
	m->n_ord += n_rec;
	return -1;
}

/* dup[0, records added) and stats[0, NABWA_MARKDUP_N_STATS) for everything added; returns the records added */
extern "C" int64_t emu_markdup_resolve(void *h, uint8_t *dup, uint64_t *stats)
{
	EmuMarkdup *m = (EmuMarkdup*)h;
	const int64_t n = (int64_t)m->n_tup;
	std::vector<uint32_t> idx((size_t)n);
	std::iota(idx.begin(), idx.end(), 0u);
	const std::vector<uint64_t> *cols[3] = { &m->k3, &m->lo, &m->hi };
	for (const std::vector<uint64_t> *c : cols) std::stable_sort(idx.begin(), idx.end(), [c](uint32_t a, uint32_t b) { return (*c)[a] < (*c)[b]; });
	std::vector<uint8_t> d((size_t)m->n_ord, 0);
	m->stats[NABWA_MARKDUP_STAT_DUP_FRAGMENTS] = m->stats[NABWA_MARKDUP_STAT_DUP_PAIRS] = m->stats[NABWA_MARKDUP_STAT_DUP_RECORDS] = 0;
	for (int64_t j = 0; j < n; ++j) md_mark_one(j, idx.data(), m->hi.data(), m->lo.data(), m->k3.data(), d.data(), m->stats);
	for (int64_t o = 0; o < m->n_ord; ++o) md_prop_one(o, m->link.data(), d.data(), m->stats);
	if (m->n_ord) memcpy(dup, d.data(), (size_t)m->n_ord);
	for (int k = 0; k < NABWA_MARKDUP_N_STATS; ++k) stats[k] = m->stats[k];
	return m->n_ord;
}
