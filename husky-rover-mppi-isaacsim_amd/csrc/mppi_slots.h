// The two slot policies of the step engine, as decisions on integers only (no HIP header, so
// tests/native/slot_policy_check.cpp checks them on the host): which normals slot holds which
// Philox step and which may be overwritten, and which tail slot the next deferred optimal rollout
// takes.  A wrong slot here means a rollout reading half-written normals.  The events, streams and
// buffers of the slots live in the parts that embed these (NormalsSlots, TailRing in mppi_ctx.h).
#pragma once
#include <cstdint>

namespace mppi {

// sampling normals, one slot per step in flight: the rollout's, the next step's and the one
// after (generated two steps ahead, so the noise kernel is never on the step's path)
constexpr int kEpsSlots = 3;

struct EpsPolicy {
  // A step is any uint64_t (the step counter is a full word of the Philox counter and
  // wraps at 2^64), so no 64-bit value can stand for "none".  The slot keeps the step in a wider signed
  // word: 0 .. 2^64 - 1 is the step it holds, -1 is none, and no step aliases it.
  using held_t = __int128;
  held_t step[kEpsSlots] = {-1, -1, -1};            // the Philox step whose normals the slot holds (-1: none)
  bool pending[kEpsSlots] = {false, false, false};  // its fill is in flight: the slot's event tells when it is done

  // The slot that holds `s`, or -1.  (No two slots hold one step: a step is generated only when
  // find() misses.  Of equal entries the highest index is returned.)
  int find(uint64_t s) const {
    int slot = -1;
    for (int i = 0; i < kEpsSlots; ++i)
      if (step[i] == (held_t)s) slot = i;
    return slot;
  }
  bool holds(uint64_t s) const { return find(s) >= 0; }
  // A slot other than `used` that holds none of the steps in (s, s + 2], taken modulo 2^64: the
  // stalest one (its last reader is a rollout enqueued before the current one).  -1: none.
  int victim(int used, uint64_t s) const {
    for (int i = 0; i < kEpsSlots; ++i) {
      if (i == used) continue;
      if (step[i] >= 0 && (uint64_t)((uint64_t)step[i] - s - 1) < 2) continue;
      return i;
    }
    return -1;
  }
  void mark_pending(int i, uint64_t s) {  // a fill of step s was enqueued and its event recorded
    step[i] = (held_t)s;
    pending[i] = true;
  }
  void mark_ready(int i, uint64_t s) {  // holds s with no event to wait for (ordered by its stream, or by the server)
    step[i] = (held_t)s;
    pending[i] = false;
  }
  void settled(int i) { pending[i] = false; }  // the fill's event was waited for
  void invalidate(int i) { step[i] = -1; }
  void forget_steps() {  // no slot holds a step (pending fills stay pending: they still write)
    for (int i = 0; i < kEpsSlots; ++i) step[i] = -1;
  }
  void invalidate_all() {  // the buffers are gone
    for (int i = 0; i < kEpsSlots; ++i) {
      step[i] = -1;
      pending[i] = false;
    }
  }
};

// Ring of N tail slots.  `latest` is the slot of the last tail launched; a server step's tail is
// `deferred` (kept on the host until its completion word was seen) in `def_slot`, the slot after.
template <int N>
struct TailRingPolicy {
  int latest = 0;         // slot of the latest tail
  bool pending = false;   // the latest tail's outputs are not merged into the host outputs yet
  bool deferred = false;  // a server step's tail waits on the host
  int def_slot = 0;
  bool inflight[N] = {};  // the tail of that slot may still run

  // The slot the next tail takes: after the deferred one when there is one, else after the latest.
  int next() const { return ((deferred ? def_slot : latest) + 1) % N; }
  void claim(int s) {  // a tail was launched into s
    inflight[s] = true;
    latest = s;
    pending = true;
  }
  void done(int s) { inflight[s] = false; }
  void all_done() {
    for (int i = 0; i < N; ++i) inflight[i] = false;
  }
  bool busy() const {  // a tail may still run, or the latest one's outputs wait to be merged
    bool any = pending;
    for (int i = 0; i < N; ++i) any |= inflight[i];
    return any;
  }
  bool must_wait(int i) const { return inflight[i] || (pending && i == latest); }
};

}  // namespace mppi
