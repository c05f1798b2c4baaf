// bam_front_main.cpp -- test harness for the host-only units of the BAM front-end (csrc/bam_rec.hpp, bam_front.cpp, host_pool.cpp,
// read_trim.hpp): no GPU, no libnabwa.  tests/test_bam_front.py builds it plain, with -fsanitize=address,undefined and with
// -fsanitize=thread, and compares what it writes with a Python model and with the reference's own answers (tests/golden/vectors_bam_front.npz).
//   front <bytes> <offsets> <flags> <trim_qual> <out>   the create stages over a record stream (bamlib.pack's layout), everything they leave -> out
//   edit  <bytes> <offsets> <script> <out>              record i gets line i of the script (revcom | cigar n c.. | pushi XY v | pushc XY c | pushs XY s ; ...)
//   reg2bin beg end [beg end ...]                       the bins
//   trim  <quals> <offsets> <trim_qual>                 per read: the shared trim function in the three callers' quality domains, then their old loops
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sstream>
#include <string>
#include <vector>
#include "../../network-aware-bwa_amd/csrc/bam_front.cpp"
#include "../../network-aware-bwa_amd/csrc/host_pool.cpp"

static std::string g_last;
int nabwa_fail(int code, const char *fmt, const char *a)          /* the library's (nabwa_api.hip), kept small: the last message */
{
	char b[1024]; snprintf(b, sizeof b, fmt, a); g_last = b;
	return code;
}

static std::vector<uint8_t> slurp(const char *fn)
{
	std::vector<uint8_t> v;
	FILE *f = fopen(fn, "rb");
	if (!f) { fprintf(stderr, "cannot read %s\n", fn); exit(3); }
	uint8_t buf[65536]; size_t k;
	while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
	fclose(f);
	return v;
}
static std::vector<int64_t> offsets(const char *fn)
{
	const std::vector<uint8_t> raw = slurp(fn);
	std::vector<int64_t> o(raw.size() / 8);
	if (!o.empty()) memcpy(o.data(), raw.data(), o.size() * 8);
	return o;
}

struct Out {
	FILE *f;
	explicit Out(const char *fn) : f(fopen(fn, "wb")) { if (!f) { fprintf(stderr, "cannot write %s\n", fn); exit(3); } }
	~Out() { fclose(f); }
	void bytes(const void *p, size_t n) { if (n) fwrite(p, 1, n, f); }
	void i32(int32_t x) { bytes(&x, 4); }
	void i64(int64_t x) { bytes(&x, 8); }
};

/* the records as nabwa_bam_batch_output writes them: n + 1 offsets, then the bytes */
template <class Recs> static void put_records(Out &o, const Recs &rec, size_t n)
{
	std::vector<int64_t> at(n + 1, 0);
	for (size_t i = 0; i < n; ++i) at[i + 1] = at[i] + 36 + (int64_t)rec[i].data.size();
	std::vector<uint8_t> buf((size_t)at[n] + 1);
	for (size_t i = 0; i < n; ++i) write_rec(rec[i], buf.data() + at[i]);
	o.bytes(at.data(), 8 * (n + 1)); o.bytes(buf.data(), (size_t)at[n]);
}

static int front(const char *fb, const char *fo, uint32_t flags, int trim_qual, const char *fout)
{
	const std::vector<uint8_t> in = slurp(fb);
	const std::vector<int64_t> off = offsets(fo);
	const int n_in = (int)off.size() - 1;
	nabwa_bam_batch b;
	memset(&b.opt, 0, sizeof b.opt); memset(&b.popt, 0, sizeof b.popt);
	b.opt.trim_qual = trim_qual; b.flags = flags;
	uint32_t any_flag = 0;
	int rc = bam_front_parse(&b, n_in, in.data(), off.data(), &any_flag);
	if (rc == NABWA_OK) rc = bam_front_pair(&b, any_flag);
	if (rc == NABWA_OK) { bam_front_read_groups(&b); rc = bam_front_encode(&b); }
	Out o(fout);
	o.i32(rc);
	if (rc != NABWA_OK) { o.bytes(g_last.data(), g_last.size()); return 0; }
	const size_t n = b.rec.size(), nk = b.kind.size();
	o.i32((int32_t)n); o.i32((int32_t)nk); o.i32((int32_t)b.rg_names.size());
	for (size_t k = 0; k < nk; ++k) { o.i32(b.kind[k]); o.i32(b.first[k]); o.i32(b.rg[k]); o.i32(b.skip[k]); }
	for (const std::string &s : b.rg_names) { o.i32((int32_t)s.size()); o.bytes(s.data(), s.size()); }
	o.bytes(b.off.data(), 8 * (n + 1)); o.bytes(b.full_len.data(), 4 * n);
	o.bytes(b.seq.data(), (size_t)b.off[n]); o.bytes(b.rseq.data(), (size_t)b.off[n]);
	put_records(o, b.rec, n);
	return 0;
}

static void edit_one(BamRec &r, const std::string &line)
{
	std::stringstream all(line); std::string op;
	while (std::getline(all, op, ';')) {
		std::stringstream s(op); std::string what, key, val;
		s >> what;
		if (what == "revcom") revcom_rec(r);
		else if (what == "cigar") { int n; s >> n; std::vector<uint32_t> c((size_t)n + 1); for (int i = 0; i < n; ++i) s >> c[i]; set_cigar(r, n, c.data()); }
		else if (what == "pushi") { long v; s >> key >> v; push_int(r, key[0], key[1], (int)v); }
		else if (what == "pushc") { s >> key >> val; push_char(r, key[0], key[1], val[0]); }
		else if (what == "pushs") { s >> key >> val; push_str(r, key[0], key[1], val.c_str()); }
		else if (!what.empty()) { fprintf(stderr, "unknown edit %s\n", what.c_str()); exit(3); }
	}
}

static int edit(const char *fb, const char *fo, const char *fs, const char *fout)
{
	const std::vector<uint8_t> in = slurp(fb), script = slurp(fs);
	const std::vector<int64_t> off = offsets(fo);
	const size_t n = off.size() - 1;
	std::vector<std::string> lines;
	{ std::stringstream s(std::string(script.begin(), script.end())); std::string l; while (std::getline(s, l)) lines.push_back(l); }
	std::vector<uint8_t> arena((size_t)(off[n] - off[0]) + n * REC_ROOM + 64);
	std::vector<BamRec> rec(n);
	for (size_t i = 0; i < n; ++i) {
		if (!parse_rec(in.data() + off[i], off[i + 1] - off[i], rec[i], arena.data() + (off[i] - off[0]) + i * (size_t)(REC_ROOM - 36))) { fprintf(stderr, "record %zu does not parse\n", i); return 3; }
		edit_one(rec[i], i < lines.size() ? lines[i] : std::string());
	}
	Out o(fout);
	put_records(o, rec, n);
	return 0;
}

/* the three spellings of bwa_trim_read the library had, each in its caller's quality domain: the model of bwa_trimmed_len */
static int old_bam_batch(const uint8_t *ql, int L, bool rev, int trim_qual)
{
	int sc = 0, mx = 0, max_l = L - 1;
	for (int l = L - 1; l >= 35 - 1; --l) {
		const int jj = rev ? L - 1 - l : l; const int q = ql[jj] + 33 < 126 ? ql[jj] : 93;
		sc += trim_qual - q;
		if (sc < 0) break;
		if (sc > mx) { mx = sc; max_l = l; }
	}
	return max_l + 1;
}
static int old_read_input(const char *q, int full, int trim_qual)
{
	int sum = 0, best = 0, best_l = full - 1;
	for (int l = full - 1; l >= 35 - 1; --l) {
		sum += trim_qual - ((int)(unsigned char)q[l] - 33);
		if (sum < 0) break;
		if (sum > best) { best = sum; best_l = l; }
	}
	return best_l + 1;
}
static int old_encode_read(const uint8_t *q, int full_len, int trim_qual)
{
	int s = 0, mx = 0, max_l = full_len - 1;
	for (int l = full_len - 1; l >= 35 - 1; --l) {
		s += trim_qual - (int)q[l];
		if (s < 0) break;
		if (s > mx) { mx = s; max_l = l; }
	}
	return max_l + 1;
}

static int trim(const char *fq, const char *fo, int trim_qual)
{
	const std::vector<uint8_t> q = slurp(fq);
	const std::vector<int64_t> off = offsets(fo);
	for (size_t i = 0; i + 1 < off.size(); ++i) {
		const uint8_t *ql = q.data() + off[i]; const int L = (int)(off[i + 1] - off[i]);
		std::string chars((size_t)L, 0);                   /* phred + 33 capped at 126, as the tools' BAM reader hands it on */
		for (int l = 0; l < L; ++l) chars[l] = (char)(ql[l] + 33 < 126 ? ql[l] + 33 : 126);
		for (int rev = 0; rev < 2; ++rev)
			printf("%d %d ", bwa_trimmed_len(L, trim_qual, [&](int l) { const int v = ql[rev ? L - 1 - l : l]; return v + 33 < 126 ? v : 93; }), old_bam_batch(ql, L, rev != 0, trim_qual));
		printf("%d %d ", bwa_trimmed_len(L, trim_qual, [&](int l) { return (int)(unsigned char)chars[l] - 33; }), old_read_input(chars.data(), L, trim_qual));
		printf("%d %d\n", bwa_trimmed_len(L, trim_qual, [&](int l) { return (int)ql[l]; }), old_encode_read(ql, L, trim_qual));
	}
	return 0;
}

int main(int argc, char **argv)
{
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "front" && argc == 7) return front(argv[2], argv[3], (uint32_t)atoi(argv[4]), atoi(argv[5]), argv[6]);
	if (what == "edit" && argc == 6) return edit(argv[2], argv[3], argv[4], argv[5]);
	if (what == "reg2bin" && argc >= 4) { for (int i = 2; i + 1 < argc; i += 2) printf("%u\n", reg2bin((uint32_t)strtoul(argv[i], 0, 10), (uint32_t)strtoul(argv[i + 1], 0, 10))); return 0; }
	if (what == "trim" && argc == 5) return trim(argv[2], argv[3], atoi(argv[4]));
	return 2;
}
