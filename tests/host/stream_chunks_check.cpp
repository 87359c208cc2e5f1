// The order of csrc/slstream.h's stream_chunks and put_all's write loop, checked on the host alone: this program
// includes only the header's HIP-free part and is built by a plain C++ compiler with the address and undefined-
// behaviour sanitizers (tests/test_host_stream.py).  Exit status 0: every check held.
#include <pthread.h>
#include <signal.h>
#include <stdio.h>
#include <string.h>
#include <sys/time.h>

#include <algorithm>
#include <string>
#include <vector>

#include "slstream.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                              \
  do {                                                \
    if (!(cond)) {                                    \
      ++failures;                                     \
      printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                            \
      printf("\n");                                   \
    }                                                 \
  } while (0)

enum Kind { kEnqueue, kLanded, kSink, kNone };
const char* const kNames[] = {"enqueue", "landed", "sink", "none"};

struct Event {
  Kind kind;
  int64_t k;  // (landed: the chunk the slot holds, in call order)
  int slot;
  bool ok;
};

// stream_chunks over recording callbacks; the `fail_at`-th call (from 0) of kind `fail` returns false
int run(int64_t n_chunks, int ring, Kind fail, int fail_at, std::vector<Event>* ev) {
  int calls[3] = {0, 0, 0};
  int64_t landed_k = 0;
  auto answer = [&](Kind kind) { return !(kind == fail && calls[kind]++ == fail_at); };
  return slstream::stream_chunks(
      n_chunks, ring,
      [&](int64_t k, int slot) {
        const bool ok = answer(kEnqueue);
        ev->push_back({kEnqueue, k, slot, ok});
        return ok;
      },
      [&](int slot) {
        const bool ok = answer(kLanded);
        ev->push_back({kLanded, landed_k++, slot, ok});
        return ok;
      },
      [&](int64_t k, int slot) {
        const bool ok = answer(kSink);
        ev->push_back({kSink, k, slot, ok});
        return ok;
      });
}

int64_t position(const std::vector<Event>& ev, Kind kind, int64_t k) {
  for (size_t i = 0; i < ev.size(); ++i)
    if (ev[i].kind == kind && ev[i].k == k) return static_cast<int64_t>(i);
  return -1;
}

int count(const std::vector<Event>& ev, Kind kind) {
  int c = 0;
  for (const Event& e : ev) c += e.kind == kind;
  return c;
}

void check_clean(int64_t n, int ring) {
  std::vector<Event> ev;
  const int r = run(n, ring, kNone, 0, &ev);
  CHECK(r == SL_OK, "n=%lld ring=%d: %d", (long long)n, ring, r);
  CHECK(static_cast<int64_t>(ev.size()) == 3 * n, "n=%lld ring=%d: %zu events", (long long)n, ring, ev.size());
  for (int kind = 0; kind < 3; ++kind) {  // every kind once per chunk, in chunk order
    int64_t next = 0;
    for (const Event& e : ev)
      if (e.kind == kind) {
        CHECK(e.k == next, "n=%lld ring=%d: %s of %lld, expected %lld", (long long)n, ring, kNames[kind],
              (long long)e.k, (long long)next);
        CHECK(e.slot == e.k % ring, "n=%lld ring=%d: %s %lld in slot %d", (long long)n, ring, kNames[kind],
              (long long)e.k, e.slot);
        ++next;
      }
    CHECK(next == n, "n=%lld ring=%d: %lld %s calls", (long long)n, ring, (long long)next, kNames[kind]);
  }
  for (int64_t k = 0; k < n; ++k) {
    const int64_t q = position(ev, kEnqueue, k), l = position(ev, kLanded, k), s = position(ev, kSink, k);
    CHECK(0 <= q && q < l && l < s, "n=%lld ring=%d: chunk %lld at %lld %lld %lld", (long long)n, ring, (long long)k,
          (long long)q, (long long)l, (long long)s);
    if (k + ring < n)
      CHECK(position(ev, kEnqueue, k + ring) > s, "n=%lld ring=%d: chunk %lld queued before %lld was sunk",
            (long long)n, ring, (long long)(k + ring), (long long)k);
  }
}

void check_failure(int64_t n, int ring, Kind fail, int fail_at) {
  std::vector<Event> ev;
  const int r = run(n, ring, fail, fail_at, &ev);
  const int want = fail == kSink ? SL_EIO : SL_EHIP;
  CHECK(r == want, "n=%lld ring=%d %s #%d: %d", (long long)n, ring, kNames[fail], fail_at, r);
  size_t at = ev.size();
  for (size_t i = 0; i < ev.size(); ++i)
    if (!ev[i].ok) {
      CHECK(at == ev.size(), "n=%lld ring=%d %s #%d: two failures", (long long)n, ring, kNames[fail], fail_at);
      at = std::min(at, i);
    }
  CHECK(at < ev.size() && ev[at].kind == fail, "n=%lld ring=%d %s #%d: the failure was never reached", (long long)n,
        ring, kNames[fail], fail_at);
  int64_t queued = 0;
  for (size_t i = 0; i < ev.size(); ++i) {
    if (ev[i].kind == kEnqueue && ev[i].ok) ++queued;
    if (i > at) {
      CHECK(ev[i].kind != kEnqueue, "n=%lld ring=%d %s #%d: chunk %lld queued after the failure", (long long)n, ring,
            kNames[fail], fail_at, (long long)ev[i].k);
      CHECK(ev[i].kind != kSink, "n=%lld ring=%d %s #%d: chunk %lld sunk after the failure", (long long)n, ring,
            kNames[fail], fail_at, (long long)ev[i].k);
    }
  }
  CHECK(count(ev, kLanded) == queued, "n=%lld ring=%d %s #%d: %lld queued, %d waited for", (long long)n, ring,
        kNames[fail], fail_at, (long long)queued, count(ev, kLanded));
  for (int64_t k = 0; k < queued; ++k)
    CHECK(position(ev, kLanded, k) > position(ev, kEnqueue, k), "n=%lld ring=%d %s #%d: chunk %lld", (long long)n,
          ring, kNames[fail], fail_at, (long long)k);
}

// ---- put_all through a pipe whose reader drains in small pieces, under a 1 ms timer signal: write(2) blocks,
// comes back short and with EINTR, and every byte still arrives once, in order
struct Reader {
  int fd;
  std::string got;
};

void* drain(void* p) {
  Reader* r = static_cast<Reader*>(p);
  char buf[1531];
  for (;;) {
    const ssize_t n = read(r->fd, buf, sizeof(buf));
    if (n < 0 && errno == EINTR) continue;
    if (n <= 0) break;
    r->got.append(buf, static_cast<size_t>(n));
  }
  return nullptr;
}

void on_alarm(int) {}

void check_put_all() {
  std::string data(3 << 20, '\0');
  for (size_t i = 0; i < data.size(); ++i) data[i] = static_cast<char>((i * 2654435761u) >> 13);
  int fds[2];
  CHECK(pipe(fds) == 0, "pipe");
  sigset_t alarm_only, before;
  sigemptyset(&alarm_only);
  sigaddset(&alarm_only, SIGALRM);
  pthread_sigmask(SIG_BLOCK, &alarm_only, &before);  // the reader inherits the mask: the writer takes the signals
  Reader reader{fds[0], {}};
  pthread_t th;
  CHECK(pthread_create(&th, nullptr, drain, &reader) == 0, "pthread_create");
  pthread_sigmask(SIG_SETMASK, &before, nullptr);
  struct sigaction sa = {}, old_sa;
  sa.sa_handler = on_alarm;  // (no SA_RESTART: a blocked write returns short or with EINTR)
  sigaction(SIGALRM, &sa, &old_sa);
  const itimerval tick = {{0, 1000}, {0, 1000}}, off = {{0, 0}, {0, 0}};
  setitimer(ITIMER_REAL, &tick, nullptr);
  const bool ok = slstream::put_all(fds[1], data.data(), data.size());
  setitimer(ITIMER_REAL, &off, nullptr);
  sigaction(SIGALRM, &old_sa, nullptr);
  CHECK(ok, "put_all into the pipe");
  CHECK(slstream::put_all(fds[1], data.data(), 0), "put_all of nothing");
  close(fds[1]);
  pthread_join(th, nullptr);
  close(fds[0]);
  CHECK(reader.got == data, "%zu bytes arrived of %zu", reader.got.size(), data.size());
  // a reader that is gone, a descriptor that is none: false, not a loop
  signal(SIGPIPE, SIG_IGN);
  CHECK(pipe(fds) == 0, "pipe");
  close(fds[0]);
  CHECK(!slstream::put_all(fds[1], data.data(), 100), "put_all into a pipe without a reader");
  close(fds[1]);
  CHECK(!slstream::put_all(-1, data.data(), 100), "put_all to no descriptor");
}

}  // namespace

int main() {
  int runs = 0;
  for (int64_t n : {0, 1, 2, 3, 7})
    for (int ring : {1, 2, 3}) {
      check_clean(n, ring);
      ++runs;
      for (Kind fail : {kEnqueue, kLanded, kSink})
        for (int at = 0; at < n; ++at, ++runs) check_failure(n, ring, fail, at);
    }
  check_put_all();
  printf("%d runs of stream_chunks, put_all: %d failed checks\n", runs, failures);
  return failures ? 1 : 0;
}
