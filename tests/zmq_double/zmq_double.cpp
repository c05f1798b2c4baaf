// zmq_double.cpp -- a stand-in for libzmq that plays `bwa bam2bam -p` inside the process that loads it: the calls nabwa_worker binds
// (libzmq 3.2 / 4.x names), no socket, no thread, no network.  Test code: tests/zmq_double/__init__.py compiles it and writes what it reads.
//
// The scenario is a directory, $ZMQ_DOUBLE_DIR:
//   config.bin     the reply to a REQ message that starts with \0 (gap_opt_t . pe_opt_t . prefix)
//   isize.bin      the reply to one that starts with \1 (may be missing or empty: no estimates yet)
//   messages.bin   the records the master has to hand out: u32 length + message, repeated
//   steps.txt      one step per line, taken in order; a step that cannot be completed yet waits for the worker's next call
//                    send N           queue the next N records of messages.bin for the DEALER connections
//                    echo             queue every answer received since the last echo, as a master sends a positioned record out again
//                    wait N           until N more answers have come in than the waits before this one took
//                    broadcast FILE   the bytes of FILE (in the directory) to every SUB socket
//                    terminate        \1 + "done" to every SUB socket
// Queued records go to the DEALER connections in turn, and never more to one than its ZMQ_RCVHWM allows (default 1000, as libzmq's).
// Out: replies.bin (every message sent over a DEALER, same framing, in the order sent) and log.txt, one event per line:
//   socket ID TYPE | setsockopt ID OPTION VALUE | connect ID ADDRESS | hello ID HEX | close ID | unknown-step ... |
//   max_outstanding N (the most records handed out and not yet answered) | max_queued N (the most that waited in one connection) | delivered N | replies N | ctx_new or init | term
// Nothing here waits: a poll that finds nothing returns 0 at once, whatever its timeout -- nothing can arrive while the caller sleeps.
#include <errno.h>
#include <stdarg.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <deque>
#include <string>
#include <vector>

namespace {
typedef std::vector<uint8_t> Bytes;
struct Msg { uint8_t *data; size_t size; };                         /* what this double keeps in the caller's 64-byte zmq_msg_t */
struct Sock { int id, type, rcvhwm; bool connected; std::deque<Bytes> q; Bytes pending; };
struct Step { std::string op, arg; long n; };

struct World {
	std::string dir; FILE *log = 0, *replies = 0;
	Bytes config, isize; std::vector<Bytes> messages; std::vector<Step> steps;
	std::vector<Sock*> socks; int next_id = 1;
	std::deque<Bytes> outbox; std::vector<Bytes> answers;
	size_t step = 0, next_msg = 0, echoed = 0, waited = 0, turn = 0;
	long outstanding = 0, max_outstanding = 0, max_queued = 0, delivered = 0; bool summed = false;
	int err = 0;
	~World() { sum_up(); }
	void say(const char *fmt, ...) __attribute__((format(printf, 2, 3)))
	{
		if (!log) return;
		va_list ap; va_start(ap, fmt); vfprintf(log, fmt, ap); va_end(ap);
		fputc('\n', log); fflush(log);
	}
	void sum_up()
	{
		if (!log || summed) return;
		summed = true;
		say("max_outstanding %ld", max_outstanding); say("max_queued %ld", max_queued); say("delivered %ld", delivered); say("replies %zu", answers.size());
	}
};
World W;

bool slurp(const std::string &path, Bytes &out)
{
	FILE *f = fopen(path.c_str(), "rb");
	if (!f) return false;
	uint8_t buf[65536]; size_t n;
	while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
	fclose(f);
	return true;
}

void load()
{
	const char *d = getenv("ZMQ_DOUBLE_DIR");
	W.dir = d ? d : ".";
	W.log = fopen((W.dir + "/log.txt").c_str(), "w");
	W.replies = fopen((W.dir + "/replies.bin").c_str(), "wb");
	slurp(W.dir + "/config.bin", W.config);
	slurp(W.dir + "/isize.bin", W.isize);
	Bytes all;
	slurp(W.dir + "/messages.bin", all);
	for (size_t p = 0; p + 4 <= all.size(); ) {
		uint32_t n; memcpy(&n, &all[p], 4);
		if (p + 4 + n > all.size()) break;
		W.messages.emplace_back(all.begin() + p + 4, all.begin() + p + 4 + n);
		p += 4 + (size_t)n;
	}
	Bytes st;
	slurp(W.dir + "/steps.txt", st);
	std::string text(st.begin(), st.end());
	for (size_t p = 0; p < text.size(); ) {
		size_t e = text.find('\n', p); if (e == std::string::npos) e = text.size();
		const std::string line = text.substr(p, e - p);
		p = e + 1;
		if (line.empty()) continue;
		const size_t sp = line.find(' ');
		Step s; s.op = line.substr(0, sp); s.arg = sp == std::string::npos ? "" : line.substr(sp + 1); s.n = atol(s.arg.c_str());
		W.steps.push_back(s);
	}
}

void to_subscribers(const Bytes &b) { for (Sock *s : W.socks) if (s && s->type == 2 && s->connected) s->q.push_back(b); }

/* the master's side: as far as the steps go without the worker doing something first */
void pump()
{
	for (;;) {
		/* hand out what is queued, a record per connection in turn, none beyond a connection's high-water mark */
		std::vector<Sock*> dealers;
		for (Sock *s : W.socks) if (s && s->type == 5 && s->connected) dealers.push_back(s);
		while (!W.outbox.empty() && !dealers.empty()) {
			Sock *to = 0;
			for (size_t k = 0; k < dealers.size() && !to; ++k) { Sock *s = dealers[(W.turn + k) % dealers.size()]; if ((long)s->q.size() < (long)s->rcvhwm) { to = s; W.turn = (W.turn + k + 1) % dealers.size(); } }
			if (!to) break;
			to->q.push_back(std::move(W.outbox.front())); W.outbox.pop_front();
			++W.delivered;
			if ((long)to->q.size() > W.max_queued) W.max_queued = (long)to->q.size();
			if (++W.outstanding > W.max_outstanding) W.max_outstanding = W.outstanding;
		}
		if (!W.outbox.empty() || W.step >= W.steps.size()) return;
		Step &s = W.steps[W.step];
		if (s.op == "send") { for (long i = 0; i < s.n && W.next_msg < W.messages.size(); ++i) W.outbox.push_back(W.messages[W.next_msg++]); }
		else if (s.op == "echo") { for (; W.echoed < W.answers.size(); ++W.echoed) W.outbox.push_back(W.answers[W.echoed]); }
		else if (s.op == "wait") { if ((long)(W.answers.size() - W.waited) < s.n) return; W.waited += (size_t)s.n; }
		else if (s.op == "broadcast") { Bytes b; slurp(W.dir + "/" + s.arg, b); to_subscribers(b); }
		else if (s.op == "terminate") { const char t[] = "\1done"; to_subscribers(Bytes(t, t + 5)); }
		else W.say("unknown-step %s %s", s.op.c_str(), s.arg.c_str());
		++W.step;
	}
}

Msg *M(void *m) { return (Msg*)m; }
void drop(Msg *m) { free(m->data); m->data = 0; m->size = 0; }
void fill(Msg *m, const Bytes &b) { drop(m); m->size = b.size(); m->data = (uint8_t*)malloc(b.size() ? b.size() : 1); if (b.size()) memcpy(m->data, b.data(), b.size()); }
int fail(int e) { W.err = e; errno = e; return -1; }
const char *type_name(int t) { return t == 2 ? "SUB" : t == 3 ? "REQ" : t == 5 ? "DEALER" : "OTHER"; }
}

extern "C" {
/* the context: libzmq 3.2 / 4.x names, or with ZMQ_DOUBLE_OLD_NAMES only the older pair that 3.x still has */
#ifndef ZMQ_DOUBLE_OLD_NAMES
void *zmq_ctx_new(void) { load(); W.say("ctx_new"); return &W; }
int zmq_ctx_term(void *) { W.sum_up(); W.say("term"); return 0; }
#else
void *zmq_init(int) { load(); W.say("init"); return &W; }
int zmq_term(void *) { W.sum_up(); W.say("term"); return 0; }
#endif
int zmq_errno(void) { return W.err; }
const char *zmq_strerror(int e) { return strerror(e); }

void *zmq_socket(void *, int type)
{
	Sock *s = new Sock(); s->id = W.next_id++; s->type = type; s->rcvhwm = 1000; s->connected = false;
	W.socks.push_back(s);
	W.say("socket %d %s", s->id, type_name(type));
	return s;
}
int zmq_close(void *sock)
{
	Sock *s = (Sock*)sock;
	W.say("close %d", s->id);
	for (Sock *&x : W.socks) if (x == s) x = 0;
	delete s;
	return 0;
}
int zmq_connect(void *sock, const char *addr) { Sock *s = (Sock*)sock; s->connected = true; W.say("connect %d %s", s->id, addr); return 0; }
int zmq_setsockopt(void *sock, int opt, const void *val, size_t len)
{
	Sock *s = (Sock*)sock;
	int v = 0;
	if (len == sizeof(int)) memcpy(&v, val, sizeof v);
	W.say("setsockopt %d %d %d", s->id, opt, len == sizeof(int) ? v : (int)len);
	if (opt == 24 && len == sizeof(int)) s->rcvhwm = v > 0 ? v : 0x7fffffff;          /* ZMQ_RCVHWM; 0 = no limit */
	return 0;
}

int zmq_msg_init(void *m) { M(m)->data = 0; M(m)->size = 0; return 0; }
int zmq_msg_init_size(void *m, size_t n) { M(m)->size = n; M(m)->data = (uint8_t*)malloc(n ? n : 1); return M(m)->data ? 0 : fail(ENOMEM); }
void *zmq_msg_data(void *m) { return M(m)->data; }
size_t zmq_msg_size(void *m) { return M(m)->size; }
int zmq_msg_close(void *m) { drop(M(m)); return 0; }

int zmq_msg_send(void *m, void *sock, int)
{
	Sock *s = (Sock*)sock; Msg *x = M(m);
	const int n = (int)x->size;
	if (s->type == 3) {                                                  /* REQ: a hello; the reply waits for the recv that follows */
		std::string hex;
		for (size_t i = 0; i < x->size; ++i) { char b[3]; snprintf(b, sizeof b, "%02x", x->data[i]); hex += b; }
		W.say("hello %d %s", s->id, hex.c_str());
		s->pending = x->size && x->data[0] == 1 ? W.isize : W.config;
	} else if (s->type == 5) {
		const uint32_t len = (uint32_t)x->size;
		if (W.replies) { fwrite(&len, 4, 1, W.replies); fwrite(x->data, 1, x->size, W.replies); fflush(W.replies); }
		W.answers.emplace_back(x->data, x->data + x->size);
		--W.outstanding;
	} else return fail(ENOTSUP);
	drop(x);
	return n;
}
int zmq_msg_recv(void *m, void *sock, int)
{
	Sock *s = (Sock*)sock;
	if (s->type == 3) { fill(M(m), s->pending); return (int)M(m)->size; }
	pump();
	if (s->q.empty()) return fail(EAGAIN);                                /* (a blocking receive would never come back: nothing runs but the caller) */
	fill(M(m), s->q.front()); s->q.pop_front();
	return (int)M(m)->size;
}

#ifndef ZMQ_DOUBLE_NO_POLL
typedef struct { void *socket; int fd; short events; short revents; } pollitem;
int zmq_poll(pollitem *it, int n, long)
{
	pump();
	int ready = 0;
	for (int i = 0; i < n; ++i) {
		Sock *s = (Sock*)it[i].socket;
		it[i].revents = (short)((it[i].events & 1) && s && !s->q.empty() ? 1 : 0);
		if (it[i].revents) ++ready;
	}
	return ready;
}
#endif
}
