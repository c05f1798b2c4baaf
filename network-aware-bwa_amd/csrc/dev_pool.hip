// dev_pool.hip -- the per-index pool of device working buffers and the staged upload (dev_pool.hpp).
#include <hip/hip_runtime.h>
#include <string.h>
#include <thread>
#include "dev_pool.hpp"
#include "host_util.hpp"

hipError_t staged_upload(nabwa_index *ix, const UploadJob *jobs, int n_jobs)
{
	nabwa_dev_pool *pl = ix->pool;
	size_t total = 0;
	for (int j = 0; j < n_jobs; ++j) total += jobs[j].bytes;
	const int T = nabwa_dev_pool::UP_THREADS; const size_t SLOT = nabwa_dev_pool::UP_SLOT;
	if (total < ((size_t)env_int("NABWA_STAGED_MIN_MB", 256) << 20) || total == 0) {       /* small: not worth four threads */
		for (int j = 0; j < n_jobs; ++j)
			if (jobs[j].bytes) { hipError_t e = hipMemcpy(jobs[j].dst, jobs[j].src, jobs[j].bytes, hipMemcpyHostToDevice); if (e != hipSuccess) return e; }
		return hipSuccess;
	}
	std::lock_guard<std::mutex> lk(pl->mu);                  /* one staged upload at a time per index */
	if (!pl->pin) {
		hipError_t e = hipHostMalloc((void**)&pl->pin, (size_t)T * 2 * SLOT, hipHostMallocDefault);
		if (e != hipSuccess) { pl->pin = 0; return e; }
		for (int t = 0; t < T; ++t) {
			if ((e = hipStreamCreateWithFlags(&pl->up_stream[t], hipStreamNonBlocking)) != hipSuccess) return e;
			for (int k = 0; k < 2; ++k) if ((e = hipEventCreateWithFlags(&pl->up_ev[t][k], hipEventDisableTiming)) != hipSuccess) return e;
		}
	}
	struct Piece { uint8_t *dst; const uint8_t *src; size_t bytes; };
	std::vector<Piece> pieces;
	for (int j = 0; j < n_jobs; ++j)
		for (size_t o = 0; o < jobs[j].bytes; o += SLOT)
			pieces.push_back({ (uint8_t*)jobs[j].dst + o, (const uint8_t*)jobs[j].src + o, jobs[j].bytes - o < SLOT ? jobs[j].bytes - o : SLOT });
	hipError_t err[T];
	std::vector<std::thread> th;
	for (int t = 0; t < T; ++t) {
		err[t] = hipSuccess;
		th.emplace_back([&, t]() {
			hipError_t e = hipSetDevice(ix->device);
			int used = 0;
			for (size_t i = t; i < pieces.size() && e == hipSuccess; i += T, ++used) {
				const int k = used & 1;
				uint8_t *slot = pl->pin + ((size_t)t * 2 + k) * SLOT;
				if (used >= 2) e = hipEventSynchronize(pl->up_ev[t][k]);       /* the copy that last used this slot is done */
				if (e != hipSuccess) break;
				memcpy(slot, pieces[i].src, pieces[i].bytes);
				e = hipMemcpyAsync(pieces[i].dst, slot, pieces[i].bytes, hipMemcpyHostToDevice, pl->up_stream[t]);
				if (e == hipSuccess) e = hipEventRecord(pl->up_ev[t][k], pl->up_stream[t]);
			}
			const hipError_t e2 = hipStreamSynchronize(pl->up_stream[t]);
			err[t] = e != hipSuccess ? e : e2;
		});
	}
	for (auto &x : th) x.join();
	for (int t = 0; t < T; ++t) if (err[t] != hipSuccess) return err[t];
	return hipSuccess;
}

void pool_flush(nabwa_dev_pool *pl)         /* caller holds the lock */
{
	for (auto &k : pl->idle) (void)hipFree(k.p);
	pl->idle.clear(); pl->idle_bytes = 0;
}

hipError_t pool_malloc(nabwa_index *ix, void **out, size_t bytes)
{
	nabwa_dev_pool *pl = ix->pool;
	if (bytes == 0) bytes = 1;
	const size_t gran = bytes >= (8u << 20) ? (2u << 20) : 256;
	const size_t need = (bytes + gran - 1) / gran * gran;
	std::lock_guard<std::mutex> lk(pl->mu);
	size_t best = pl->idle.size();
	for (size_t i = 0; i < pl->idle.size(); ++i)
		if (pl->idle[i].bytes >= need && pl->idle[i].bytes <= need + need / 4 + 4096 && (best == pl->idle.size() || pl->idle[i].bytes < pl->idle[best].bytes)) best = i;
	if (best != pl->idle.size()) {
		*out = pl->idle[best].p; pl->live[*out] = pl->idle[best].bytes; pl->idle_bytes -= pl->idle[best].bytes;
		pl->idle.erase(pl->idle.begin() + best);
		return hipSuccess;
	}
	hipError_t e = hipMalloc(out, need);
	if (e != hipSuccess && !pl->idle.empty()) { (void)hipGetLastError(); pool_flush(pl); e = hipMalloc(out, need); }
	if (e == hipSuccess) pl->live[*out] = need;
	return e;
}

hipError_t pool_free(nabwa_index *ix, void *p)
{
	if (!p) return hipSuccess;
	nabwa_dev_pool *pl = ix->pool;
	std::lock_guard<std::mutex> lk(pl->mu);
	auto it = pl->live.find(p);
	if (it == pl->live.end()) return hipFree(p);
	const size_t bytes = it->second;
	pl->live.erase(it);
	if (bytes > pl->limit) return hipFree(p);
	pl->idle.push_back({ p, bytes }); pl->idle_bytes += bytes;
	while (pl->idle_bytes > pl->limit) {            /* the oldest go first */
		(void)hipFree(pl->idle.front().p); pl->idle_bytes -= pl->idle.front().bytes; pl->idle.erase(pl->idle.begin());
	}
	return hipSuccess;
}

nabwa_dev_pool *pool_create()
{
	nabwa_dev_pool *pl = new nabwa_dev_pool();
	pl->limit = (size_t)env_int("NABWA_POOL_GB", 80) << 30;
	return pl;
}

void pool_destroy(nabwa_dev_pool *pl)
{
	if (!pl) return;
	{ std::lock_guard<std::mutex> lk(pl->mu); pool_flush(pl); }
	if (pl->pin) (void)hipHostFree(pl->pin);
	for (int t = 0; t < nabwa_dev_pool::UP_THREADS; ++t) {
		if (pl->up_stream[t]) (void)hipStreamDestroy(pl->up_stream[t]);
		for (int k = 0; k < 2; ++k) if (pl->up_ev[t][k]) (void)hipEventDestroy(pl->up_ev[t][k]);
	}
	delete pl;
}
