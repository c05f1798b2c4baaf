// isize_table.cpp -- the nabwa_isize_table_* entry points (insert_size.c:141-213).
#include <string.h>
#include "isize_table.hpp"
#include "host_util.hpp"

extern "C" nabwa_isize_table_t *nabwa_isize_table_create(double ap_prior, int64_t genome_len)
{
	nabwa_isize_table *t = new nabwa_isize_table();
	t->ap_prior = ap_prior; t->L = genome_len; t->poscache = nabwa_poscache_create();
	return t;
}
extern "C" void nabwa_isize_table_destroy(nabwa_isize_table_t *t) { if (t) nabwa_poscache_destroy(t->poscache); delete t; }

/* improve_isize_est (insert_size.c:141-165): one logical record's contribution.  The 16-bit bins wrap as the reference's do
 * (its "hit the ceiling" test compares an unsigned short with -1 and never fires). */
nabwa_isize_table::Rg *isize_slot(nabwa_isize_table *t, const std::string &rg)
{
	auto it = t->rg.find(rg);
	if (it == t->rg.end()) {
		nabwa_isize_table::Rg r; memset(&r.ii, 0, sizeof(r.ii)); r.hist.assign(100000, 0); r.has_hist = true;
		it = t->rg.emplace(rg, std::move(r)).first;
	}
	return &it->second;
}

/* infer_all_isizes (insert_size.c:167-173): every read group that still has its histogram gets its estimate */
extern "C" int nabwa_isize_table_infer_all(nabwa_isize_table_t *t)
{
	if (!t) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (auto &kv : t->rg)
		if (kv.second.has_hist) {
			nabwa_isize_infer(kv.second.hist.data(), t->ap_prior, t->L, &kv.second.ii);
			kv.second.hist.clear(); kv.second.hist.shrink_to_fit(); kv.second.has_hist = false;
		}
	return NABWA_OK;
}

extern "C" int nabwa_isize_table_get(const nabwa_isize_table_t *t, const char *rg, nabwa_isize_t *out)
{
	if (!t || !rg || !out) return nabwa_fail(NABWA_EINVAL, "null argument");
	auto it = t->rg.find(rg);
	if (it == t->rg.end() || it->second.has_hist) { memset(out, 0, sizeof(*out)); return 1; }      /* null_ii (bam2bam.c:106,715) */
	*out = it->second.ii;
	return NABWA_OK;
}

extern "C" int nabwa_isize_table_merge(nabwa_isize_table_t *t, const nabwa_isize_table_t *other)      /* the host add between passes of N shards */
{
	if (!t || !other) return nabwa_fail(NABWA_EINVAL, "null argument");
	for (const auto &kv : other->rg) {
		if (!kv.second.has_hist) continue;
		auto it = t->rg.find(kv.first);
		if (it == t->rg.end()) { t->rg.emplace(kv.first, kv.second); continue; }
		if (!it->second.has_hist) continue;
		for (size_t b = 0; b < 100000; ++b) it->second.hist[b] = (uint16_t)(it->second.hist[b] + kv.second.hist[b]);
	}
	return NABWA_OK;
}

/* encode_iinfo / decode_iinfo (insert_size.c:185-213): the blob `bwa worker` receives -- per read group its name, NUL, then the
 * raw isize_info_t (a dead histogram pointer, then avg, std, ap_prior, low, high, high_bayesian: 48 bytes) */
extern "C" int64_t nabwa_isize_table_encode(const nabwa_isize_table_t *t, uint8_t *out, int64_t cap)
{
	if (!t) return nabwa_fail(NABWA_EINVAL, "null argument");
	int64_t need = 0;
	for (const auto &kv : t->rg) need += (int64_t)kv.first.size() + 1 + 8 + (int64_t)sizeof(nabwa_isize_t);
	if (!out || cap < need) return need;
	uint8_t *p = out;
	for (const auto &kv : t->rg) {
		memcpy(p, kv.first.c_str(), kv.first.size() + 1); p += kv.first.size() + 1;
		memset(p, 0, 8); p += 8;
		memcpy(p, &kv.second.ii, sizeof(nabwa_isize_t)); p += sizeof(nabwa_isize_t);
	}
	return need;
}
extern "C" int nabwa_isize_table_decode(nabwa_isize_table_t *t, const uint8_t *in, int64_t n)
{
	if (!t || (n && !in)) return nabwa_fail(NABWA_EINVAL, "null argument");
	const uint8_t *p = in, *q = in + n;
	while (p < q) {
		const size_t l = strnlen((const char*)p, (size_t)(q - p));
		if (p + l + 1 + 8 + sizeof(nabwa_isize_t) > q) return nabwa_fail(NABWA_EINVAL, "error when decoding isize info");
		nabwa_isize_table::Rg r; r.has_hist = false;
		memcpy(&r.ii, p + l + 1 + 8, sizeof(nabwa_isize_t));
		t->rg[std::string((const char*)p, l)] = r;
		p += l + 1 + 8 + sizeof(nabwa_isize_t);
	}
	return NABWA_OK;
}
