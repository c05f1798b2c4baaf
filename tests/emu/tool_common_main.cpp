// tool_common_main.cpp -- test harness for csrc/tool_common.hpp, the parts that need no GPU and no libnabwa: the NABWA_DEVICES parser,
// final_rename, Chan and InOrder.  The first argument names the case; a case that checks itself prints "ok" and exits 0, or says what
// it saw and exits 4.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <random>
#define TOOL "tool_common_main"
#include "../../network-aware-bwa_amd/csrc/tool_common.hpp"

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "line %d: %s\n", __LINE__, #c); fflush(stderr); _exit(4); } } while (0)
static void pause_ms(int ms) { std::this_thread::sleep_for(std::chrono::milliseconds(ms)); }

/* cap + 1 items into a channel of cap: the producer gets as far as cap and no further until one is taken; then 1000 items through it,
 * never more than cap of them waiting; then close(): a waiting get comes back false, but not before what was put is out */
static void chan(size_t cap)
{
	{
		Chan<int> ch(cap);
		std::atomic<size_t> n_put(0);
		std::thread producer([&]() { for (size_t i = 0; i <= cap; ++i) { ch.put((int)i); ++n_put; } });
		while (n_put < cap) std::this_thread::yield();
		pause_ms(50);
		CHECK(n_put == cap);
		int x = -1;
		CHECK(ch.get(x) && x == 0);
		producer.join();
		CHECK(n_put == cap + 1);
		for (size_t i = 1; i <= cap; ++i) CHECK(ch.get(x) && x == (int)i);
	}
	{
		Chan<int> ch(cap);
		std::thread producer([&]() { for (int i = 0; i < 1000; ++i) ch.put(std::move(i)); ch.close(); });
		int x, want = 0;
		for (;;) {
			{ std::unique_lock<std::mutex> l(ch.m); CHECK(ch.q.size() <= cap); }
			if (!ch.get(x)) break;
			CHECK(x == want++);
		}
		CHECK(want == 1000);
		producer.join();
	}
	{
		Chan<int> ch(cap);
		bool got = true;
		std::thread consumer([&]() { int x; got = ch.get(x); });
		pause_ms(50);
		ch.close();
		consumer.join();
		CHECK(!got);
	}
	{
		Chan<int> ch(cap);
		for (size_t i = 0; i < cap; ++i) ch.put((int)i);
		ch.close();
		int x = -1;
		for (size_t i = 0; i < cap; ++i) CHECK(ch.get(x) && x == (int)i);
		CHECK(!ch.get(x));
	}
	printf("ok\n");
}

/* how far the furthest waiting result is ahead of the one get() hands out next */
template <class T> static long lead(InOrder<T> &io) { std::unique_lock<std::mutex> l(io.m); return io.held.empty() ? 0 : io.held.rbegin()->first - io.next; }

/* four producers take the numbers 0..199, scrambled within runs of 8 (less than the bound, so the number the consumer waits for is never
 * behind one that cannot be put yet), from one list; the consumer starts once the first run waits for it */
static void inorder(long bound, unsigned seed)
{
	const int N = 200, RUN = 8;
	std::vector<long> order(N);
	for (int i = 0; i < N; ++i) order[i] = i;
	std::mt19937 rng(seed);
	for (int i = 0; i < N; i += RUN) std::shuffle(order.begin() + i, order.begin() + i + RUN, rng);
	InOrder<long> io(bound);
	std::atomic<int> at(0), working(4);
	std::atomic<long> max_lead(0);
	auto note = [&]() { const long l = lead(io); long m = max_lead; while (l > m && !max_lead.compare_exchange_weak(m, l)) {} };
	std::vector<std::thread> producers;
	for (int t = 0; t < 4; ++t)
		producers.emplace_back([&]() {
			for (int i; (i = at++) < N; ) { CHECK(io.put(order[i], 1000 + order[i])); note(); }
			if (--working == 0) io.close();
		});
	for (;;) { std::unique_lock<std::mutex> l(io.m); if ((int)io.held.size() >= RUN) break; l.unlock(); std::this_thread::yield(); }
	long want = 0, x = 0;
	for (;;) {
		note();
		if (!io.get(x)) break;
		CHECK(x == 1000 + want);
		++want;
	}
	for (auto &p : producers) p.join();
	CHECK(want == N && !io.failed());
	printf("max_lead %ld\n", (long)max_lead);
}

/* fail(): producers that wait for room and a consumer that waits for the next result all come back with false, and so does every later call */
static void inorder_fail()
{
	InOrder<int> io(2);
	bool put_ok[3] = { true, true, true }, got = true;
	std::vector<std::thread> th;
	for (int t = 0; t < 3; ++t) th.emplace_back([&, t]() { put_ok[t] = io.put(2 + t, 7); });      /* 0 and 1 never come: no room for these */
	th.emplace_back([&]() { int x; got = io.get(x); });
	pause_ms(50);
	io.fail();
	for (auto &x : th) x.join();
	int x;
	CHECK(!put_ok[0] && !put_ok[1] && !put_ok[2] && !got && io.failed() && !io.put(0, 1) && !io.get(x));
	printf("ok\n");
}

int main(int argc, char **argv)
{
	const std::string what = argc > 1 ? argv[1] : "";
	if (what == "devices") { for (int d : tool_devices()) printf("%d ", d); printf("\n"); }
	else if (what == "rename" && argc == 4) final_rename(argv[2], atoi(argv[3]) != 0);
	else if (what == "chan" && argc == 3) chan((size_t)atoi(argv[2]));
	else if (what == "inorder" && argc == 4) inorder(atol(argv[2]), (unsigned)atoi(argv[3]));
	else if (what == "inorder_fail") inorder_fail();
	else return 2;
	return 0;
}
