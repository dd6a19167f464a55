// Host check of the step engine's two slot policies (csrc/mppi_slots.h) and of the owning handles
// (csrc/mppi_handles.h, with a counting fake in place of the HIP runtime).  Built with ASan + UBSan
// by tests/test_slot_policy.py; neither header needs a HIP header here.
#define MPPI_HANDLES_NO_HIP
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

#include "mppi_handles.h"
#include "mppi_slots.h"

using namespace mppi;

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

// ---- normals slots ----
// A step is any uint64_t and the counter wraps at 2^64, so "none" is a flag beside
// the step, never a step value, and every sum or difference of steps below is modulo 2^64.
struct Held {
  bool has;
  uint64_t step;
};

// The rule as the step engine has always applied it, restated literally: the lowest index other
// than `used` that holds no step, or a step not in (s, s + 2] (d = step - s - 1 is 0 or 1), or -1.
static int victim_rule(const Held st[3], int used, uint64_t s) {
  for (int i = 0; i < 3; ++i) {
    if (i == used) continue;
    const uint64_t d = st[i].step - s - 1u;
    const bool keep = st[i].has && d < 2u;
    if (!keep) return i;
  }
  return -1;
}

// Linear search; of equal entries (never reachable: a step is generated only when the search
// misses) the highest index, as the engine's search loop had it.
static int find_linear(const Held st[3], uint64_t s) {
  int r = -1;
  for (int i = 0; i < 3; ++i)
    if (st[i].has && st[i].step == s) r = i;
  return r;
}

static void check_eps() {
  static_assert(kEpsSlots == 3, "the enumeration below is over three slots");
  const uint64_t top = ~(uint64_t)0, half = (uint64_t)1 << 63;  // 2^64 - 1, 2^63
  long states = 0, failed_before = g_fail;
  for (uint64_t s : {(uint64_t)0, (uint64_t)1000, half - 2, half - 1, half, top - 2, top - 1, top}) {
    // {none, s - 1, s, s + 1, s + 2, s + 3}; the states are set through the marks alone, as the engine does
    const Held vals[6] = {{false, 0}, {true, s - 1u}, {true, s}, {true, s + 1u}, {true, s + 2u}, {true, s + 3u}};
    for (int a = 0; a < 6; ++a)
      for (int b = 0; b < 6; ++b)
        for (int c = 0; c < 6; ++c) {
          const Held st[3] = {vals[a], vals[b], vals[c]};
          EpsPolicy p;
          for (int i = 0; i < 3; ++i)
            if (st[i].has) p.mark_ready(i, st[i].step);
          for (int used = 0; used < 3; ++used) {
            CHECK(p.victim(used, s) == victim_rule(st, used, s));
            ++states;
          }
          for (uint64_t q : {s - 1u, s, s + 1u, s + 2u, s + 3u, s + 7u}) {
            CHECK(p.find(q) == find_linear(st, q));
            CHECK(p.holds(q) == (find_linear(st, q) >= 0));
          }
        }
    if (g_fail != failed_before) {
      std::printf("  (%ld checks failed at s = 0x%016llx)\n", (long)(g_fail - failed_before), (unsigned long long)s);
      failed_before = g_fail;
    }
  }
  CHECK(states == 8 * 216 * 3);
  {  // a fresh policy holds no step at all
    EpsPolicy f;
    for (uint64_t q : {(uint64_t)0, (uint64_t)1, half - 1, half, top - 1, top}) CHECK(f.find(q) == -1 && !f.holds(q));
    for (uint64_t s : {(uint64_t)0, half - 1, top - 2, top - 1, top}) CHECK(f.victim(0, s) == 1 && f.victim(1, s) == 0);
  }
  {  // the steps over the wrap, as speculate_eps walks them: two victims for + 1 and + 2, found again
    EpsPolicy w;
    const uint64_t s = top - 2;  // 2^64 - 3
    w.mark_ready(0, s);
    const int v1 = w.victim(0, s);
    CHECK(v1 == 1);
    w.mark_pending(v1, s + 1u);
    const int v2 = w.victim(0, s);
    CHECK(v2 == 2);
    w.mark_pending(v2, s + 2u);  // step 2^64 - 1
    CHECK(w.find(s) == 0 && w.find(s + 1u) == 1 && w.find(top) == 2 && w.victim(0, s) == -1);
    // step 2^64 - 2 reads slot 1; step + 2 is step 0, into the slot of the stale 2^64 - 3
    CHECK(w.holds(top) && !w.holds(0) && w.victim(1, s + 1u) == 0);
    w.mark_pending(0, s + 3u);
    CHECK(w.find(0) == 0 && w.victim(1, s + 1u) == -1);
    // step 2^64 - 1 reads slot 2; step 0 is kept, step 1 goes over the stale 2^64 - 2
    CHECK(w.holds(0) && !w.holds(1) && w.victim(2, top) == 1);
    w.mark_pending(1, 1);
    CHECK(w.find(top) == 2 && w.find(0) == 0 && w.find(1) == 1 && w.victim(2, top) == -1);
    CHECK(w.victim(0, 0) == 2);  // at step 0, step 2^64 - 1 is stale
    w.forget_steps();
    CHECK(w.find(top) == -1 && w.find(0) == -1 && w.find(1) == -1 && !w.holds(top));
    w.mark_ready(2, top);
    w.invalidate(2);
    CHECK(w.find(top) == -1);
    w.mark_ready(2, top);
    w.invalidate_all();
    CHECK(w.find(top) == -1 && w.find(0) == -1);
  }
  // the marks
  EpsPolicy p;
  CHECK(p.find(0) == -1 && p.victim(0, 0) == 1);
  p.mark_ready(0, 5);
  p.mark_pending(1, 6);
  p.mark_pending(2, 7);
  CHECK(p.find(5) == 0 && p.find(6) == 1 && p.find(7) == 2);
  CHECK(!p.pending[0] && p.pending[1] && p.pending[2]);
  CHECK(p.victim(0, 5) == -1);  // both others hold steps in (5, 7]
  CHECK(p.victim(1, 6) == 0);   // step 5 is stale at step 6
  p.settled(1);
  CHECK(!p.pending[1] && p.step[1] == 6);
  p.invalidate(2);
  CHECK(p.find(7) == -1 && p.pending[2]);  // (its fill may still write: the event is still waited for)
  p.forget_steps();
  CHECK(p.find(5) == -1 && p.find(6) == -1 && p.pending[2]);
  p.invalidate_all();
  CHECK(!p.pending[0] && !p.pending[1] && !p.pending[2]);
}

// ---- tail ring ----
template <int N>
static void check_tail() {
  for (int latest = 0; latest < N; ++latest)
    for (int def = -1; def < N; ++def) {  // -1: no deferred tail
      TailRingPolicy<N> t;
      t.latest = latest;
      t.deferred = def >= 0;
      t.def_slot = def >= 0 ? def : 0;
      const int x = def >= 0 ? def : latest;
      CHECK(t.next() == (x + 1) % N);
    }
  TailRingPolicy<N> t;
  CHECK(!t.busy());
  const int s = t.next();
  CHECK(s == 1 % N);
  t.claim(s);
  CHECK(t.latest == s && t.pending && t.inflight[s] && t.busy() && t.must_wait(s));
  t.done(s);
  CHECK(!t.inflight[s] && t.must_wait(s));  // still the latest, and not merged
  t.pending = false;
  CHECK(!t.busy() && !t.must_wait(s));
  t.claim(t.next());
  t.claim(t.next());
  t.all_done();
  for (int i = 0; i < N; ++i) CHECK(!t.inflight[i]);
}

// ---- handles ----
struct FakeApi {
  using event_t = int*;
  using stream_t = long*;
  static int dev_allocs, dev_frees, pin_frees, event_destroys, stream_destroys;
  static bool fail_next;
  static int dev_alloc(void** p, size_t bytes) {
    if (fail_next) {
      fail_next = false;
      return 2;
    }
    *p = std::malloc(bytes ? bytes : 1);
    ++dev_allocs;
    return 0;
  }
  static void dev_free(void* p) {
    std::free(p);
    ++dev_frees;
  }
  static int pin_alloc(void** p, size_t bytes) {
    *p = std::malloc(bytes ? bytes : 1);
    return 0;
  }
  static void pin_free(void* p) {
    std::free(p);
    ++pin_frees;
  }
  static int event_create(event_t* e, unsigned) {
    *e = new int(0);
    return 0;
  }
  static void event_destroy(event_t e) {
    delete e;
    ++event_destroys;
  }
  static int stream_create(stream_t* s, unsigned) {
    *s = new long(0);
    return 0;
  }
  static int stream_create_prio(stream_t* s, unsigned, int) { return stream_create(s, 0); }
  static void stream_destroy(stream_t s) {
    delete s;
    ++stream_destroys;
  }
};
int FakeApi::dev_allocs = 0, FakeApi::dev_frees = 0, FakeApi::pin_frees = 0, FakeApi::event_destroys = 0,
    FakeApi::stream_destroys = 0;
bool FakeApi::fail_next = false;

using Buf = DeviceBufT<float, FakeApi>;
using Pin = PinnedBufT<float, FakeApi>;
using Ev = EventT<FakeApi>;
using St = StreamT<FakeApi>;

static void check_handles() {
  {  // destruction releases once; an empty handle releases nothing
    Buf a, empty;
    CHECK(a.alloc(64) == 0 && a.cap() == 64 && a.owned() && a.get());
    CHECK(!empty && empty.cap() == 0);
  }
  CHECK(FakeApi::dev_frees == 1);
  {  // move: the source is empty, one release in all
    Buf a;
    a.alloc(16);
    float* p = a;
    Buf b(std::move(a));
    CHECK(b.get() == p && b.cap() == 16 && !a.get() && a.cap() == 0 && !a.owned());
  }
  CHECK(FakeApi::dev_frees == 2);
  {  // move-assign onto a live handle releases the target's old buffer, then the moved one at the end
    Buf a, b;
    a.alloc(16);
    b.alloc(32);
    float* p = a;
    b = std::move(a);
    CHECK(FakeApi::dev_frees == 3 && b.get() == p && b.cap() == 16 && !a.get());
    Buf& self = b;
    b = std::move(self);  // self-assignment keeps it
    CHECK(b.get() == p && FakeApi::dev_frees == 3);
  }
  CHECK(FakeApi::dev_frees == 4);
  {  // reset releases once and empties; a second reset does nothing
    Buf a;
    a.alloc(8);
    a.reset();
    CHECK(FakeApi::dev_frees == 5 && !a.get() && a.cap() == 0);
    a.reset();
    CHECK(FakeApi::dev_frees == 5);
  }
  CHECK(FakeApi::dev_frees == 5);
  {  // grow: nothing within the capacity, one release of the old buffer beyond it; a failed
     // allocation leaves the handle empty with capacity 0
    Buf a;
    CHECK(a.grow(100) == 0 && FakeApi::dev_frees == 5);
    float* p = a;
    CHECK(a.grow(50) == 0 && a.get() == p && a.cap() == 100 && FakeApi::dev_frees == 5);
    CHECK(a.grow(200) == 0 && a.cap() == 200 && FakeApi::dev_frees == 6);
    FakeApi::fail_next = true;
    CHECK(a.grow(400) == 2 && !a.get() && a.cap() == 0 && FakeApi::dev_frees == 7);
  }
  CHECK(FakeApi::dev_frees == 7 && FakeApi::dev_allocs == 7);
  {  // a borrowed pointer is never released: not on reset, move, allocation over it or destruction
    float mine[4] = {};
    Buf a;
    a.borrow(mine);
    CHECK(a.get() == mine && !a.owned() && a.cap() == 0);
    Buf b(std::move(a));
    CHECK(b.get() == mine && !b.owned());
    b.reset();
    CHECK(!b.get());
    b.borrow(mine);
    CHECK(b.alloc(8) == 0 && b.owned() && b.get() != mine);  // the borrowed one is let go of
    CHECK(FakeApi::dev_frees == 7);
    b.borrow(mine);  // the owned one is released as the handle lets go of it
    CHECK(FakeApi::dev_frees == 8);
    Buf c;
    c.alloc(8);
    c = std::move(b);  // borrowed state moves with the pointer
    CHECK(FakeApi::dev_frees == 9 && c.get() == mine && !c.owned());
  }
  CHECK(FakeApi::dev_frees == 9);
  {  // pinned buffer, event, stream: once each; a borrowed stream (the caller's) never
    Pin p;
    p.alloc(32);
    Ev e;
    e.create();
    Ev e2(std::move(e));
    St s;
    s.create(0, 1);
    long callers = 0;
    St t;
    t.borrow(&callers);
    s = std::move(t);  // the owned stream is destroyed here, the caller's never
    CHECK(FakeApi::stream_destroys == 1 && s.get() == &callers && !s.owned());
    s.create(0);  // (mppi_set_stream(NULL): back to an owned stream)
    CHECK(s.owned() && FakeApi::stream_destroys == 1);
    std::vector<Ev> v;  // handles live in containers
    for (int i = 0; i < 5; ++i) {
      Ev x;
      x.create();
      v.push_back(std::move(x));
    }
  }
  CHECK(FakeApi::pin_frees == 1 && FakeApi::event_destroys == 6 && FakeApi::stream_destroys == 2);
}

int main() {
  check_eps();
  check_tail<4>();
  check_tail<3>();
  check_tail<1>();
  check_handles();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("slot policy ok\n");
  return 0;
}
