// worker_main.cpp -- `nabwa_worker`: the command line and the sockets of `bwa worker` (bam2bam.c:2213-2309, bwa_worker_core :2099-2211)
// around the library's worker core (nabwa_worker_core, wire_worker.cpp).
//
//     nabwa_worker -p PORT [-h HOST] [-t N] [-T MINUTES]
//
// Hello over a REQ socket to tcp://HOST:PORT (`\0` + nodename -> gap_opt_t . pe_opt_t . index prefix), the index of that prefix onto the GPU,
// `\1` + nodename -> the insert-size estimates the master has so far, then records over DEALER connections to PORT + 1 and broadcasts over a
// SUB socket to PORT + 2 until the master says `\1`, nothing comes for 90 s, -T minutes have passed or a signal arrives.  Host code only;
// the GPU work is the library's.
//
// libzmq is bound at run time (dlopen: $NABWA_ZMQ_LIB, libzmq.so.5, libzmq.so.3, libzmq.so): neither this program nor libnabwa.so links
// to it, and the build needs no <zmq.h> -- the few constants and the two structs used are declared below, the stable ABI of libzmq 3.2 and
// 4.x.  Without a library, or with one that lacks a call, one line says which, exit 2.
//
// Records in flight: the reference's master keeps 64 records per peer on the wire (the_hwm, bam2bam.c:35,1221-1227), a GPU batch wants
// 10^4 .. 10^6.  Two levers, neither measured against a real master: the DEALER sockets' own high-water marks are raised to
// NABWA_WORKER_INFLIGHT (65536), and -t N opens N DEALER connections, which a master that counts per peer sees as N workers.  With N > 1
// the order of arrival, and with it the drand48 stream, is not deterministic -- as with the reference's N threads.
// NABWA_WORKER_BATCH (262144) and NABWA_WORKER_LINGER_MS (5): the most records of a GPU batch, and how long to wait for more once one is there.
// NABWA_DEVICE picks the GPU.  Exit status: 0 a clean end, 1 usage / a bad reply / an error while working, 2 no usable GPU or libzmq.
#include <dlfcn.h>
#include <errno.h>
#include <getopt.h>
#include <signal.h>
#include <sys/utsname.h>
#define TOOL "nabwa_worker"
#include "tool_common.hpp"

/* ---------------------------------------------------------------- libzmq 3.2 / 4.x, as much of its ABI as is used (zmq.h of those versions) */
enum { ZMQ_SUB = 2, ZMQ_REQ = 3, ZMQ_DEALER = 5 };                                    /* socket types */
enum { ZMQ_SUBSCRIBE = 6, ZMQ_LINGER = 17, ZMQ_SNDHWM = 23, ZMQ_RCVHWM = 24 };        /* socket options */
enum { ZMQ_POLLIN = 1, ZMQ_DONTWAIT = 1 };
typedef struct { alignas(void*) unsigned char _[64]; } zmq_msg_t;                     /* 32 bytes in 3.2 / 4.0, 64 from 4.1 on: room for both */
typedef struct { void *socket; int fd; short events; short revents; } zmq_pollitem_t;

struct Zmq {
	void *(*ctx_new)(void); void *(*init)(int); int (*ctx_term)(void*); int (*term)(void*);
	void *(*socket)(void*, int); int (*close)(void*); int (*connect)(void*, const char*); int (*setsockopt)(void*, int, const void*, size_t);
	int (*msg_init)(zmq_msg_t*); int (*msg_init_size)(zmq_msg_t*, size_t); void *(*msg_data)(zmq_msg_t*); size_t (*msg_size)(zmq_msg_t*);
	int (*msg_send)(zmq_msg_t*, void*, int); int (*msg_recv)(zmq_msg_t*, void*, int); int (*msg_close)(zmq_msg_t*);
	int (*poll)(zmq_pollitem_t*, int, long); int (*zerrno)(void); const char *(*strerror)(int);
	std::string file;
	const char *why() const { return strerror(zerrno()); }
};

/* 0 = bound; otherwise the one line that says what is missing has been printed */
static int bind_zmq(Zmq &z)
{
	std::vector<std::string> names;
	if (getenv("NABWA_ZMQ_LIB") && *getenv("NABWA_ZMQ_LIB")) names.push_back(getenv("NABWA_ZMQ_LIB"));
	names.push_back("libzmq.so.5"); names.push_back("libzmq.so.3"); names.push_back("libzmq.so");
	void *h = 0; std::string tried;
	for (const std::string &n : names) {
		if ((h = dlopen(n.c_str(), RTLD_NOW | RTLD_LOCAL))) { z.file = n; break; }
		const char *e = dlerror();
		tried += (tried.empty() ? "" : "; ") + n + (e && !strstr(e, n.c_str()) ? std::string(" (") + e + ")" : "");
	}
	if (!h) { fprintf(stderr, "[nabwa_worker] no usable libzmq, cannot load any of: %s (NABWA_ZMQ_LIB names another)\n", tried.c_str()); return -1; }
	const char *missing = 0;
	auto sym = [&](const char *name, const char *older) -> void* {
		void *p = dlsym(h, name);
		if (!p && older) p = dlsym(h, older);
		if (!p && !missing) missing = name;
		return p;
	};
#define BIND(field, name, older) z.field = (decltype(z.field))sym(name, older)
	z.ctx_new = (decltype(z.ctx_new))dlsym(h, "zmq_ctx_new"); z.init = (decltype(z.init))dlsym(h, "zmq_init");
	z.ctx_term = (decltype(z.ctx_term))dlsym(h, "zmq_ctx_term"); z.term = (decltype(z.term))dlsym(h, "zmq_term");
	if (!z.ctx_new && !z.init) missing = "zmq_ctx_new";
	else if (!z.ctx_term && !z.term) missing = "zmq_ctx_term";
	BIND(socket, "zmq_socket", 0); BIND(close, "zmq_close", 0); BIND(connect, "zmq_connect", 0); BIND(setsockopt, "zmq_setsockopt", 0);
	BIND(msg_init, "zmq_msg_init", 0); BIND(msg_init_size, "zmq_msg_init_size", 0); BIND(msg_data, "zmq_msg_data", 0); BIND(msg_size, "zmq_msg_size", 0);
	BIND(msg_send, "zmq_msg_send", 0); BIND(msg_recv, "zmq_msg_recv", 0); BIND(msg_close, "zmq_msg_close", 0);
	BIND(poll, "zmq_poll", 0); BIND(zerrno, "zmq_errno", 0); BIND(strerror, "zmq_strerror", 0);
#undef BIND
	if (missing) { fprintf(stderr, "[nabwa_worker] no usable libzmq: %s has no %s (libzmq 3.2 or 4.x is needed)\n", z.file.c_str(), missing); return -1; }
	return 0;
}

/* ---------------------------------------------------------------- the work loop's transport: N DEALER sockets and one SUB socket under one poll */
static volatile sig_atomic_t s_interrupted = 0;
static void on_signal(int) { s_interrupted = 1; }

enum End { END_NONE, END_IDLE, END_TERMINATED, END_SIGNAL, END_LIFETIME, END_TRANSPORT, END_ISIZE };
struct Net {
	Zmq *z; std::vector<void*> dealers; void *sub; nabwa_worker_t *w;
	zmq_msg_t in; bool have;
	size_t next;                               /* the DEALER to look at first: the connections take turns */
	std::vector<zmq_pollitem_t> it;
	std::deque<size_t> from;                   /* which connection each unanswered record came over: its answer goes back the same way */
	double deadline; End end; std::string detail;
};

/* handle_broadcast (bam2bam.c:2079-2097): 1 = go on, 0 = the termination code, -1 = it cannot be read or its estimates cannot be decoded */
static int take_broadcast(Net *s)
{
	Zmq &z = *s->z; zmq_msg_t b;
	z.msg_init(&b);
	if (z.msg_recv(&b, s->sub, 0) < 0) { s->end = END_TRANSPORT; s->detail = std::string("receiving a broadcast failed: ") + z.why(); z.msg_close(&b); return -1; }
	const uint8_t *p = (const uint8_t*)z.msg_data(&b); const size_t n = z.msg_size(&b);
	fprintf(stderr, "[nabwa_worker] received a broadcast of %zu bytes\n", n);
	int go = 1;
	if (n == 0) ;
	else if (p[0] == 1) { s->end = END_TERMINATED; s->detail.assign((const char*)p + 1, n - 1); go = 0; }
	else if (p[0] == 2) {
		if (n > 1 && nabwa_worker_set_isize(s->w, p + 1, (int64_t)n - 1) != NABWA_OK) { s->end = END_ISIZE; s->detail = nabwa_last_error(); go = -1; }
	}
	/* anything else: the reference's handler answers -1, which its loop takes for "go on" (bam2bam.c:2096,2179) -- so does this one */
	else fprintf(stderr, "[nabwa_worker] a broadcast that starts with byte %u is none this worker knows: ignored\n", (unsigned)p[0]);
	z.msg_close(&b);
	return go;
}

static int net_recv(void *ctx, const uint8_t **msg, int64_t *len, int timeout_ms)
{
	Net *s = (Net*)ctx; Zmq &z = *s->z;
	if (s->have) { z.msg_close(&s->in); s->have = false; }
	const double until = now_s() + 1e-3 * (double)timeout_ms;
	const size_t nd = s->dealers.size();
	std::vector<zmq_pollitem_t> &it = s->it;
	it.resize(nd + 1);
	for (;;) {
		if (s_interrupted) { s->end = END_SIGNAL; return -1; }
		const double t = now_s();
		if (t >= s->deadline) { s->end = END_LIFETIME; return -1; }
		double wait = until - t; if (wait < 0) wait = 0;
		if (s->deadline - t < wait) wait = s->deadline - t;
		for (size_t i = 0; i < nd; ++i) it[i] = { s->dealers[i], 0, ZMQ_POLLIN, 0 };
		it[nd] = { s->sub, 0, ZMQ_POLLIN, 0 };
		const int np = z.poll(it.data(), (int)nd + 1, (long)(wait * 1e3 + 0.999));
		if (np < 0) {
			if (z.zerrno() == EINTR) continue;
			s->end = END_TRANSPORT; s->detail = std::string("zmq_poll failed: ") + z.why(); return -1;
		}
		if (it[nd].revents & ZMQ_POLLIN) {
			const int go = take_broadcast(s);
			if (go <= 0) return -1;
			continue;                                  /* (the estimates are in place before the next record is looked at) */
		}
		for (size_t k = 0; k < nd; ++k) {
			const size_t i = (s->next + k) % nd;
			if (!(it[i].revents & ZMQ_POLLIN)) continue;
			z.msg_init(&s->in);
			if (z.msg_recv(&s->in, s->dealers[i], ZMQ_DONTWAIT) < 0) {
				z.msg_close(&s->in);
				if (z.zerrno() == EAGAIN || z.zerrno() == EINTR) continue;
				s->end = END_TRANSPORT; s->detail = std::string("receiving a record failed: ") + z.why(); return -1;
			}
			s->have = true; s->next = (i + 1) % nd; s->from.push_back(i); s->end = END_NONE;
			*msg = (const uint8_t*)z.msg_data(&s->in); *len = (int64_t)z.msg_size(&s->in);
			return 1;
		}
		if (np == 0 && now_s() >= until) { s->end = END_IDLE; return 0; }
	}
}

static int net_send(void *ctx, const uint8_t *msg, int64_t len)
{
	Net *s = (Net*)ctx; Zmq &z = *s->z;
	size_t i = 0;
	if (!s->from.empty()) { i = s->from.front(); s->from.pop_front(); }
	zmq_msg_t m;
	if (z.msg_init_size(&m, (size_t)len) != 0) return -1;
	if (len) memcpy(z.msg_data(&m), msg, (size_t)len);
	while (z.msg_send(&m, s->dealers[i], 0) < 0) {
		if (z.zerrno() == EINTR) continue;                 /* a signal ends the loop after this batch's answers are out */
		s->end = END_TRANSPORT; s->detail = std::string("sending a record failed: ") + z.why(); z.msg_close(&m);
		return -1;
	}
	return 0;
}

static void close_now(Zmq &z, void *sock) { if (!sock) return; const int linger = 0; z.setsockopt(sock, ZMQ_LINGER, &linger, sizeof linger); z.close(sock); }

static int usage(int nthreads, const char *host, int port, int minutes)
{
	fprintf(stderr, "\nUsage:   nabwa_worker [options]\n\n");
	fprintf(stderr, "Options: -t, --num-threads NUM             number of connections to the master [%d]\n", nthreads);
	fprintf(stderr, "         -h, --host HOST                   host to connect to [%s]\n", host);
	fprintf(stderr, "         -p, --port NUM                    port to connect to [%d]\n", port);
	fprintf(stderr, "         -T, --timeout NUM                 terminate after NUM minutes [%d]\n\n", minutes);
	fprintf(stderr, "Environment: NABWA_DEVICE (the GPU, default 0), NABWA_ZMQ_LIB (the libzmq to load), NABWA_WORKER_INFLIGHT (high-water marks of\n"
					"             the connections, 65536), NABWA_WORKER_BATCH (records per GPU batch, 262144), NABWA_WORKER_LINGER_MS (wait for more, 5)\n\n");
	return 1;
}

int main(int argc, char **argv)
{
	static struct option longopts[] = { { "num-threads", 1, 0, 't' }, { "host", 1, 0, 'h' }, { "port", 1, 0, 'p' }, { "timeout", 1, 0, 'T' }, { 0, 0, 0, 0 } };
	int c, nthreads = 1, port = 0, minutes = 90;
	const char *host = "localhost";
	while ((c = getopt_long(argc, argv, "t:h:p:T:", longopts, 0)) >= 0) {
		switch (c) {
			case 't': nthreads = atoi(optarg); break;
			case 'h': host = optarg; break;
			case 'p': port = atoi(optarg); break;
			case 'T': minutes = atoi(optarg); break;
			default: return 1;
		}
	}
	if (optind != argc || port <= 0 || port > 65533) return usage(nthreads, host, port, minutes);
	if (nthreads < 1) nthreads = 1;
	if (nthreads > 64) { fprintf(stderr, "[nabwa_worker] -t %d: at most 64 connections\n", nthreads); return 1; }
	if (!tool_dedup_ok()) return 1;      /* NABWA_DEDUP: the worker core's search batches read it (include/nabwa.h) */
	const double t_start = now_s();

	Zmq z{};
	if (bind_zmq(z) != 0) return 2;
	void *zctx = z.ctx_new ? z.ctx_new() : z.init(1);
	if (!zctx) { fprintf(stderr, "[nabwa_worker] %s: no context: %s\n", z.file.c_str(), z.why()); return 2; }
	auto end_ctx = [&]() { if (z.ctx_term) z.ctx_term(zctx); else z.term(zctx); };
	{
		struct sigaction sa; memset(&sa, 0, sizeof sa);
		sa.sa_handler = on_signal; sigemptyset(&sa.sa_mask);               /* no SA_RESTART: a waiting poll comes back with EINTR */
		sigaction(SIGINT, &sa, 0); sigaction(SIGTERM, &sa, 0);
	}

	/* ---- the start-up exchange (bam2bam.c:2250-2299) */
	struct utsname un; uname(&un);
	const std::string node = un.nodename;
	char addr[300];
	void *conf = z.socket(zctx, ZMQ_REQ);
	snprintf(addr, sizeof addr, "tcp://%s:%d", host, port);
	auto fail_conf = [&](const char *what, const char *why) { fprintf(stderr, "[nabwa_worker] %s %s: %s\n", what, addr, why); close_now(z, conf); end_ctx(); return 1; };
	if (!conf || z.connect(conf, addr) != 0) return fail_conf("cannot connect to", z.why());
	auto ask = [&](char code, std::vector<uint8_t> &reply) -> bool {
		zmq_msg_t m;
		if (z.msg_init_size(&m, node.size() + 1) != 0) return false;
		uint8_t *d = (uint8_t*)z.msg_data(&m); d[0] = (uint8_t)code; memcpy(d + 1, node.data(), node.size());
		if (z.msg_send(&m, conf, 0) < 0) { z.msg_close(&m); return false; }
		z.msg_init(&m);
		if (z.msg_recv(&m, conf, 0) < 0) { z.msg_close(&m); return false; }
		const uint8_t *p = (const uint8_t*)z.msg_data(&m);
		reply.assign(p, p + z.msg_size(&m));
		z.msg_close(&m);
		return true;
	};
	std::vector<uint8_t> reply;
	if (!ask(0, reply)) return fail_conf("no configuration from", z.why());
	nabwa_gap_opt_t go; nabwa_pe_opt_t po; char prefix[4096];
	if (nabwa_wire_config_decode(reply.data(), (int64_t)reply.size(), &go, &po, prefix, sizeof prefix) != NABWA_OK)
		return fail_conf("a configuration that cannot be read from", nabwa_last_error()[0] ? nabwa_last_error() : "an index prefix of 4 KB or more");
	/* the library's limits, as nabwa_bam2bam states them for its own command line */
	if (po.max_occ_se < 0 || po.max_occ_se > NABWA_MAX_MULTI - 1 || po.n_multi < 0 || po.n_multi > NABWA_MAX_MULTI || po.N_multi < 0 || po.N_multi > NABWA_MAX_MULTI || go.s_mm < 1 || go.s_gapo < 1 || go.s_gape < 1)
		return fail_conf("options beyond the library's limits from", "-D 0..15, -h / -H 0..16, -M / -O / -E at least 1");
	fprintf(stderr, "[nabwa_worker] %s: configuration from %s, index %s\n", node.c_str(), addr, prefix);

	int device;
	if (!tool_device(&device, "")) { close_now(z, conf); end_ctx(); return 2; }
	nabwa_index_t *ix = 0; nabwa_worker_t *w = 0;
	int rc = nabwa_index_load(prefix, device, 1, 1, &ix);
	if (rc == NABWA_OK) rc = nabwa_worker_create(ix, &go, &po, &w);
	if (rc != NABWA_OK) {
		fprintf(stderr, "[nabwa_worker] loading the index %s failed: %s\n", prefix, nabwa_last_error());
		if (ix) nabwa_index_destroy(ix);
		close_now(z, conf); end_ctx();
		return rc == NABWA_ENODEV || rc == NABWA_ENOMEM ? 2 : 1;
	}
	fprintf(stderr, "[nabwa_worker] index on GPU %d after %.1f s\n", device, now_s() - t_start);
	if (!ask(1, reply)) { nabwa_worker_destroy(w); nabwa_index_destroy(ix); return fail_conf("no answer to the second hello from", z.why()); }
	if (!reply.empty() && nabwa_worker_set_isize(w, reply.data(), (int64_t)reply.size()) != NABWA_OK) {
		nabwa_worker_destroy(w); nabwa_index_destroy(ix);
		return fail_conf("insert-size estimates that cannot be read from", nabwa_last_error());
	}
	close_now(z, conf);

	/* ---- the work loop (bam2bam.c:2099-2197): DEALER connection(s) to port + 1, SUB to port + 2; the reference's second DEALER is its inproc
	 * fan-out to threads and has no counterpart here */
	Net net; net.z = &z; net.sub = 0; net.w = w; net.have = false; net.next = 0; net.end = END_NONE;
	net.deadline = t_start + 60.0 * (double)minutes;
	const int inflight = env_int("NABWA_WORKER_INFLIGHT", 65536, 1);
	bool up = true;
	for (int i = 0; i < nthreads && up; ++i) {
		void *d = z.socket(zctx, ZMQ_DEALER);
		if (d) net.dealers.push_back(d);
		snprintf(addr, sizeof addr, "tcp://%s:%d", host, port + 1);
		up = d && z.setsockopt(d, ZMQ_SNDHWM, &inflight, sizeof inflight) == 0 && z.setsockopt(d, ZMQ_RCVHWM, &inflight, sizeof inflight) == 0 && z.connect(d, addr) == 0;
	}
	if (up) {
		net.sub = z.socket(zctx, ZMQ_SUB);
		snprintf(addr, sizeof addr, "tcp://%s:%d", host, port + 2);
		up = net.sub && z.connect(net.sub, addr) == 0 && z.setsockopt(net.sub, ZMQ_SUBSCRIBE, "", 0) == 0;
	}
	int status = 0;
	if (!up) { fprintf(stderr, "[nabwa_worker] cannot connect to %s: %s\n", addr, z.why()); status = 1; }
	else {
		nabwa_worker_opt_t wo;
		wo.max_batch = env_int("NABWA_WORKER_BATCH", 262144, 1); wo.linger_ms = env_int("NABWA_WORKER_LINGER_MS", 5, 0); wo.idle_timeout_ms = 90000;      /* timeout, bam2bam.c:10 */
		rc = nabwa_worker_core(w, net_recv, net_send, &net, &wo);
		if (rc != NABWA_OK) { fprintf(stderr, "[nabwa_worker] stopped by an error: %s%s%s\n", nabwa_last_error(), net.detail.empty() ? "" : " -- ", net.detail.c_str()); status = 1; }
		else switch (net.end) {
			case END_TERMINATED: fprintf(stderr, "[nabwa_worker] received the termination signal: \"%s\"\n", net.detail.c_str()); break;
			case END_SIGNAL: fprintf(stderr, "[nabwa_worker] received an interrupt signal\n"); break;
			case END_LIFETIME: fprintf(stderr, "[nabwa_worker] %d minutes have passed (-T): done\n", minutes); break;
			case END_TRANSPORT: case END_ISIZE: fprintf(stderr, "[nabwa_worker] stopped by an error: %s\n", net.detail.c_str()); status = 1; break;
			default: fprintf(stderr, "[nabwa_worker] no work delivered in 90 s: done\n"); break;
		}
	}
	if (net.have) z.msg_close(&net.in);
	close_now(z, net.sub);
	for (void *d : net.dealers) close_now(z, d);
	end_ctx();
	uint64_t cnt[4] = { 0, 0, 0, 0 };
	nabwa_worker_counts(w, cnt);
	fprintf(stderr, "[nabwa_worker] records: %llu positioned, %llu finished, %llu bounced (no estimates), %llu passed through; %.1f s\n",
			(unsigned long long)cnt[0], (unsigned long long)cnt[1], (unsigned long long)cnt[2], (unsigned long long)cnt[3], now_s() - t_start);
	nabwa_worker_destroy(w);
	tool_dedup_cache_summary({ ix });
	nabwa_index_destroy(ix);
	return status;
}
