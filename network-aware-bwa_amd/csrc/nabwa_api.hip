// nabwa_api.hip -- what the host units of libnabwa.so share and the entries that belong to none of them: the last-error string,
// the option defaults, and bwa_cal_sa_reg_gap as one call.  The index lives in nabwa_index.hip, the search batch in nabwa_batch.hip,
// the device pool in dev_pool.hip.  Plain HIP runtime calls; no torch, no CPU fallback of the compute path.
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <math.h>
#include <string>
#include "../../include/nabwa.h"
#include "nabwa_internal.hpp"
#include "host_util.hpp"

static thread_local std::string g_err;
static int fail(int code, const char *fmt, const char *a = "")
{
	char buf[512]; snprintf(buf, sizeof buf, fmt, a); g_err = buf; return code;
}
int nabwa_fail(int code, const char *fmt, const char *a) { return fail(code, fmt, a); }

extern "C" const char *nabwa_last_error(void) { return g_err.c_str(); }

extern "C" int nabwa_device_count(void)
{
	int n = 0;
	if (hipGetDeviceCount(&n) != hipSuccess) return 0;
	return n;
}

extern "C" void nabwa_gap_init_opt(nabwa_gap_opt_t *o)   /* gap_init_opt, bwtaln.c:19-35 */
{
	memset(o, 0, sizeof(*o));
	o->s_mm = 3; o->s_gapo = 11; o->s_gape = 4;
	o->max_diff = -1; o->max_gapo = 1; o->max_gape = 6;
	o->indel_end_skip = 5; o->max_del_occ = 10; o->max_entries = 2000000;
	o->mode = NABWA_MODE_GAPE | NABWA_MODE_COMPREAD;
	o->seed_len = 32; o->max_seed_diff = 2;
	o->fnr = 0.04f; o->n_threads = 1; o->max_top2 = 30; o->trim_qual = 0;
}

/* bwa_cal_maxdiff (bwtaln.c:37-49): Poisson tail with the reference's int factorial, which
 * wraps past 12!; evaluated on the host in double, same expression order. */
extern "C" int nabwa_cal_maxdiff(int l, double err, double thres)
{
	double elambda = exp(-l * err), sum = elambda, y = 1.0;
	uint32_t x = 1;
	for (int k = 1; k < 1000; ++k) {
		y *= l * err;
		x *= (uint32_t)k;
		sum += elambda * y / (int32_t)x;
		if (1.0 - sum < thres) return k;
	}
	return 2;
}

extern "C" int nabwa_cal_sa_reg_gap(nabwa_index_t *ix, const nabwa_gap_opt_t *opt, int n, const int64_t *off,
									const uint8_t *seq, const uint8_t *rseq, int per_read,
									int32_t *n_aln, nabwa_aln1_t *aln_out, int64_t aln_cap, int64_t *n_rows,
									int32_t *max_entries)
{
	nabwa_batch_t *b = 0;
	const bool timing = getenv("NABWA_TIMING") != 0;
	const double t0 = now_s();
	if (n_rows) *n_rows = 0;
	int r = nabwa_batch_create(ix, opt, n, off, seq, rseq, per_read, &b);
	if (r != NABWA_OK) return r;
	const double t1 = now_s();
	r = nabwa_batch_run(b);
	if (r == NABWA_OK) r = nabwa_batch_sync(b, 0);
	const double t2 = now_s();
	if (r == NABWA_OK) r = nabwa_batch_fetch(b, n_aln, aln_out, aln_cap, n_rows, max_entries);
	else if (r == NABWA_EHITS) {      /* a few reads have more hit rows than NABWA_ALNCAP2: every other read's result is still handed out */
		const std::string msg = g_err;
		const int r2 = nabwa_batch_fetch(b, n_aln, aln_out, aln_cap, n_rows, max_entries);
		if (r2 != NABWA_OK) r = r2; else g_err = msg;
	}
	const double t3 = now_s();
	nabwa_batch_destroy(b);
	if (timing) fprintf(stderr, "[nabwa] cal_sa_reg_gap %d reads: upload + layout %.3f s, kernels %.3f s, compaction + download %.3f s, release %.3f s\n",
						n, t1 - t0, t2 - t1, t3 - t2, now_s() - t3);
	return r;
}
