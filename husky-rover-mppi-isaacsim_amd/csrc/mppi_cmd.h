// The resident step server's command and its wire form (no HIP includes: the host-side pack and
// the snapshot predicate also build stand-alone, tests/native/cmd_wire_check.cpp).
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define MPPI_CMD_HD __host__ __device__
#else
#define MPPI_CMD_HD
#endif

namespace mppi {

// One step's command as the host composes it and as a workgroup keeps it in LDS.
struct ServerCmd {
  unsigned seq;    // the step's completion sequence number
  unsigned stop;   // (word 1 is not part of a command: its wire slot is the stop word)
  int eps_slot;    // normals slot of the step
  int cur;         // nominal buffer the step reads (the finish writes the other one)
  int tail_slot;   // deferred optimal rollout slot (mode 2)
  int mode;        // 1: finish with the whole optimal rollout, 2: step 0 only (the rest deferred)
  int noise_slot;  // >= 0: the rollout workgroups outside the finish generate the normals of Philox block
                   // base noise_n_base into this slot after their records (-1: none)
  unsigned noise_n_base_lo;
  float x0, y0, h0x, h0y, h0z, wl, wr, gx, gy, s1, s2, igx, igy, pf_scale;  // robot / goal state
  int pf_far, speed_on;
  unsigned noise_n_base_hi;
  unsigned pad1[7];
};
constexpr int kCmdWords = 25;  // the words a step reads (seq .. noise_n_base_hi)

// Wire form, host -> head (pinned host memory) and head -> the other workgroups (device memory):
// slot i of kCmdWords naturally aligned 8-byte words holds {command word i, seq << 32}, each written
// by ONE 8-byte store, so a reader tells from the data alone whether it holds the whole command: it
// loads every slot in one sweep and accepts when all tags agree and are not before the sequence
// number it expects.  No word's validity rests on the order of two stores or on the sweep being
// atomic: a sweep that caught the writer half way holds two different tags and is taken again.
// Slot kCmdStopSlot is no command word: its low half is the launch id of the launch that is to end
// (host: mppi_capi.cpp post_stop; relay: the head as it leaves), never cleared, examined before the tags.
constexpr int kCmdSlots = 32;
constexpr int kCmdStopSlot = 1;
struct ServerCmdWire {
  uint64_t slot[kCmdSlots];
};

MPPI_CMD_HD inline uint64_t cmd_pair(unsigned word, unsigned seq) { return ((uint64_t)seq << 32) | word; }
MPPI_CMD_HD inline unsigned cmd_word(uint64_t pair) { return (unsigned)pair; }
MPPI_CMD_HD inline unsigned cmd_tag(uint64_t pair) { return (unsigned)(pair >> 32); }

// Slot i of a sweep whose slot 0 carries the tag seq0: is it part of an acceptable command?
MPPI_CMD_HD inline bool cmd_slot_ok(int i, uint64_t pair, unsigned seq0, unsigned expect) {
  return i == kCmdStopSlot || (cmd_tag(pair) == seq0 && (int)(seq0 - expect) >= 0);
}
MPPI_CMD_HD inline bool cmd_stop_hit(uint64_t stop_slot, unsigned launch_id) { return cmd_word(stop_slot) == launch_id; }

// The wire slots of command d for step seq (slot kCmdStopSlot is left alone).
inline void cmd_pack(const ServerCmd& d, unsigned seq, uint64_t out[kCmdWords]) {
  const unsigned* dw = reinterpret_cast<const unsigned*>(&d);
  for (int i = 0; i < kCmdWords; ++i)
    if (i != kCmdStopSlot) out[i] = cmd_pair(i == 0 ? seq : dw[i], seq);
}

// Post it: one 8-byte atomic store per slot, in any order (release: whatever the host wrote for the
// step before is visible to a device that sees a slot).
inline void cmd_post(ServerCmdWire* w, const ServerCmd& d, unsigned seq) {
  uint64_t p[kCmdWords];
  cmd_pack(d, seq, p);
  for (int i = 0; i < kCmdWords; ++i)
    if (i != kCmdStopSlot) __atomic_store_n(&w->slot[i], p[i], __ATOMIC_RELEASE);
}

// What a reader makes of one sweep of the kCmdWords slots (the server's wave computes the same
// from cmd_stop_hit and cmd_slot_ok, a slot per lane): the stop first, then the tags.
enum CmdVerdict { kCmdWait = 0, kCmdAccept = 1, kCmdStop = 2 };
inline CmdVerdict cmd_check(const uint64_t snap[kCmdWords], unsigned expect, unsigned launch_id) {
  if (cmd_stop_hit(snap[kCmdStopSlot], launch_id)) return kCmdStop;
  const unsigned seq0 = cmd_tag(snap[0]);
  for (int i = 0; i < kCmdWords; ++i)
    if (!cmd_slot_ok(i, snap[i], seq0, expect)) return kCmdWait;
  return kCmdAccept;
}

}  // namespace mppi
