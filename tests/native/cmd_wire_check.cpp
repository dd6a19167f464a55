// Host check of the resident server's command wire form (csrc/mppi_cmd.h): cmd_post packs a command
// into tagged 8-byte slots, cmd_check is the reader's verdict on one sweep of them.  Built with
// -fsanitize=address,undefined by tests/test_cmd_wire.py; prints "cmd wire ok" and exits 0.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "mppi_cmd.h"

using namespace mppi;

static int failures = 0;
#define CHECK(x)                                                  \
  do {                                                            \
    if (!(x)) {                                                   \
      std::printf("FAIL line %d: %s\n", __LINE__, #x);            \
      ++failures;                                                 \
    }                                                             \
  } while (0)

static ServerCmd make_cmd(unsigned salt) {
  ServerCmd d;
  std::memset(&d, 0, sizeof(d));
  unsigned* w = reinterpret_cast<unsigned*>(&d);
  for (int i = 0; i < kCmdWords; ++i) w[i] = 0x9e3779b9u * (salt + 1) + 0x01010101u * (unsigned)i;
  return d;
}

int main() {
  static_assert(sizeof(ServerCmd) == 4 * kCmdSlots, "ServerCmd is kCmdSlots words");
  static_assert(sizeof(ServerCmdWire) == 8 * kCmdSlots, "one 8-byte slot per word");
  static_assert(kCmdWords <= kCmdSlots && kCmdStopSlot < kCmdWords, "slots");
  const unsigned launch = 7, other_launch = 6;
  for (unsigned seq : {1u, 2u, 1000u, 0x7fffffffu, 0x80000000u, 0xffffffffu, 0u}) {
    const unsigned prev = seq - 1;
    ServerCmdWire* w = new ServerCmdWire;
    std::memset(w, 0, sizeof(*w));
    w->slot[kCmdStopSlot] = other_launch;  // an earlier launch's stop, never cleared
    const ServerCmd before = make_cmd(prev), d = make_cmd(seq);
    cmd_post(w, before, prev);
    // the previous step's command is complete but lies before `expect`
    CHECK(cmd_check(w->slot, seq, launch) == kCmdWait);
    CHECK(cmd_check(w->slot, prev, launch) == kCmdAccept);
    cmd_post(w, d, seq);
    CHECK(w->slot[kCmdStopSlot] == other_launch);  // posting leaves the stop slot alone
    // a complete snapshot is accepted, as the step itself or as a later one than expected
    CHECK(cmd_check(w->slot, seq, launch) == kCmdAccept);
    CHECK(cmd_check(w->slot, prev, launch) == kCmdAccept);
    CHECK(cmd_check(w->slot, seq + 1, launch) == kCmdWait);  // tags agree but lie before expect
    // it carries the command's words (word 0 the seq), and the tag in every slot
    const unsigned* dw = reinterpret_cast<const unsigned*>(&d);
    for (int i = 0; i < kCmdWords; ++i) {
      if (i == kCmdStopSlot) continue;
      CHECK(cmd_word(w->slot[i]) == (i == 0 ? seq : dw[i]));
      CHECK(cmd_tag(w->slot[i]) == seq);
    }
    // any one word still carrying the previous step's tag: rejected, whatever is expected
    uint64_t old_pairs[kCmdWords];
    cmd_pack(before, prev, old_pairs);
    for (int i = 0; i < kCmdWords; ++i) {
      if (i == kCmdStopSlot) continue;
      uint64_t snap[kCmdWords];
      std::memcpy(snap, w->slot, sizeof(snap));
      snap[i] = old_pairs[i];
      CHECK(cmd_check(snap, seq, launch) == kCmdWait);
      CHECK(cmd_check(snap, prev, launch) == kCmdWait);
      // and the other way round: one new word among the previous step's
      uint64_t mixed[kCmdWords];
      std::memcpy(mixed, old_pairs, sizeof(mixed));
      mixed[kCmdStopSlot] = other_launch;
      mixed[i] = w->slot[i];
      CHECK(cmd_check(mixed, seq, launch) == kCmdWait);
      CHECK(cmd_check(mixed, prev, launch) == kCmdWait);
    }
    // the stop is honoured before the seq: with a complete command, with a stale or a mixed one
    uint64_t snap[kCmdWords];
    std::memcpy(snap, w->slot, sizeof(snap));
    snap[kCmdStopSlot] = launch;
    CHECK(cmd_check(snap, seq, launch) == kCmdStop);
    CHECK(cmd_check(snap, seq + 1, launch) == kCmdStop);
    snap[3] = old_pairs[3];
    CHECK(cmd_check(snap, seq, launch) == kCmdStop);
    // another launch's id in the stop slot stops nothing, whatever its upper half holds
    snap[3] = w->slot[3];
    snap[kCmdStopSlot] = ((uint64_t)launch << 32) | other_launch;
    CHECK(cmd_check(snap, seq, launch) == kCmdAccept);
    delete w;
  }
  if (failures) return 1;
  std::printf("cmd wire ok\n");
  return 0;
}
