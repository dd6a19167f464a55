// Host check of the bookkeeping of a batch's per-episode scenes and trajectory counts
// (csrc/mppi_batch_scene.h).  Built with ASan + UBSan by tests/test_batch_scene_book.py; the header
// needs no HIP header.
#include <cstdint>
#include <cstdio>

#include "mppi_batch_scene.h"

using namespace mppi;

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static const SceneGeom kDem{400, 400, -20.0f, -20.0f, 0.1f};
static const SceneGeom kDemOther{1500, 1500, -75.0f, -75.0f, 0.1f};
static const SceneGeom kCm{400, 0, 20.0f, 0.1f, 0.0f};
static const SceneGeom kCmOther{750, 0, 75.0f, 0.2f, 0.0f};

static void check_blocks() {
  CHECK(BatchSceneBook::blocks_for(1) == 1);
  CHECK(BatchSceneBook::blocks_for(256) == 1);
  CHECK(BatchSceneBook::blocks_for(257) == 2);
  CHECK(BatchSceneBook::blocks_for(512) == 2);
  CHECK(BatchSceneBook::blocks_for(4096) == 16);
  BatchSceneBook b(4, 256, 1024, 512);
  for (int e = 0; e < 4; ++e) {  // the default record: the context's scene and K
    const SceneRecord r = b.record(e);
    CHECK(r.dem == -1 && r.cm == -1 && r.K == 512 && r.blocks == 2);
  }
  const int64_t ks[4] = {1, 256, 257, 512};
  const int want[4] = {1, 1, 2, 2};
  for (int e = 0; e < 4; ++e) {
    CHECK(b.set_episode_K(e, ks[e]) == kSceneOk);
    CHECK(b.record(e).K == (int32_t)ks[e] && b.record(e).blocks == want[e]);
  }
  CHECK(b.set_episode_K(0, 513) == kSceneKRange);
  CHECK(b.set_episode_K(0, -1) == kSceneKRange);
  CHECK(b.record(0).K == 1);  // a refused call changes nothing
  CHECK(b.set_episode_K(4, 1) == kSceneEpisode);
  CHECK(b.set_episode_K(-1, 1) == kSceneEpisode);
  CHECK(b.set_episode_K(0, 0) == kSceneOk);
  CHECK(b.record(0).K == 512 && b.record(0).blocks == 2 && b.K_of(0) == 512);
}

static void check_slots() {
  BatchSceneBook b(3, 256, 1024, 512);
  CHECK(b.slots(kSceneDem) == 256 && b.slots(kSceneCostmap) == 1024);
  // range
  CHECK(b.set_slot(kSceneDem, 256, kDem) == kSceneSlotRange);
  CHECK(b.set_slot(kSceneDem, -1, kDem) == kSceneSlotRange);
  CHECK(b.set_slot(kSceneCostmap, 1024, kCm) == kSceneSlotRange);
  CHECK(b.free_slot(kSceneCostmap, 1024) == kSceneSlotRange);
  CHECK(!b.live(kSceneDem, 256) && !b.live(kSceneDem, 0));
  // an episode cannot take an empty slot, or one outside the table; nothing changes
  SceneKind bad = kSceneCostmap;
  CHECK(b.set_episode_scene(0, 5, -1, &bad) == kSceneSlotEmpty && bad == kSceneDem);
  CHECK(b.set_episode_scene(0, -1, 7, &bad) == kSceneSlotEmpty && bad == kSceneCostmap);
  CHECK(b.set_episode_scene(0, 256, -1, &bad) == kSceneSlotRange && bad == kSceneDem);
  CHECK(b.set_episode_scene(0, -2, -1, &bad) == kSceneSlotRange && bad == kSceneDem);
  CHECK(b.set_episode_scene(0, -1, 1024, &bad) == kSceneSlotRange && bad == kSceneCostmap);
  CHECK(b.set_episode_scene(3, -1, -1) == kSceneEpisode);
  CHECK(b.dem_of(0) == -1 && b.costmap_of(0) == -1);
  // set, hold, replace, free
  CHECK(b.set_slot(kSceneDem, 5, kDem) == kSceneOk && b.live(kSceneDem, 5));
  CHECK(b.set_slot(kSceneCostmap, 1023, kCm) == kSceneOk && b.live(kSceneCostmap, 1023));
  CHECK(b.set_episode_scene(1, 5, 1023) == kSceneOk);
  CHECK(b.record(1).dem == 5 && b.record(1).cm == 1023);
  // a valid DEM with an empty costmap changes neither
  CHECK(b.set_episode_scene(2, 5, 3, &bad) == kSceneSlotEmpty && bad == kSceneCostmap);
  CHECK(b.dem_of(2) == -1 && b.costmap_of(2) == -1);
  int who = -1;
  CHECK(b.free_slot(kSceneDem, 5, &who) == kSceneSlotHeld && who == 1);
  who = -1;
  CHECK(b.free_slot(kSceneCostmap, 1023, &who) == kSceneSlotHeld && who == 1);
  CHECK(b.live(kSceneDem, 5) && b.live(kSceneCostmap, 1023));
  CHECK(b.set_slot(kSceneDem, 5, kDem) == kSceneOk);  // replaced while held
  CHECK(b.set_episode_scene(1, -1, 1023) == kSceneOk);
  CHECK(b.free_slot(kSceneDem, 5) == kSceneOk && !b.live(kSceneDem, 5));
  CHECK(b.free_slot(kSceneDem, 5) == kSceneOk);  // freeing an empty slot is no error
  CHECK(b.set_episode_scene(0, 5, -1) == kSceneSlotEmpty);
  CHECK(b.set_episode_scene(1, -1, -1) == kSceneOk);
  CHECK(b.free_slot(kSceneCostmap, 1023) == kSceneOk && !b.live(kSceneCostmap, 1023));
}

static void check_table() {
  BatchSceneBook b(3, 256, 1024, 512);
  CHECK(!b.need_table());
  CHECK(b.set_slot(kSceneDem, 0, kDem) == kSceneOk);
  CHECK(b.set_slot(kSceneCostmap, 2, kCm) == kSceneOk);
  CHECK(!b.need_table());  // live slots nobody holds
  CHECK(b.set_episode_scene(1, 0, -1) == kSceneOk);
  CHECK(!b.need_table() && !b.any_costmap_held());  // held by an episode that was never set
  b.mark_set(0);
  CHECK(!b.need_table());
  b.mark_set(1);
  CHECK(b.need_table() && !b.any_costmap_held());
  CHECK(b.set_episode_scene(1, -1, -1) == kSceneOk);
  CHECK(!b.need_table());  // the last holder reset
  CHECK(b.set_episode_K(0, 300) == kSceneOk);
  CHECK(b.need_table());
  CHECK(b.set_episode_K(0, 0) == kSceneOk);
  CHECK(!b.need_table());
  CHECK(b.set_episode_scene(0, -1, 2) == kSceneOk);
  CHECK(b.need_table() && b.any_costmap_held());
  CHECK(b.set_episode_K(0, 512) == kSceneOk);  // the context's K given explicitly still counts as held
  CHECK(b.set_episode_scene(0, -1, -1) == kSceneOk);
  CHECK(b.need_table() && !b.any_costmap_held());
  CHECK(b.set_episode_K(0, 0) == kSceneOk);
  CHECK(!b.need_table());
}

static void check_geometry() {
  BatchSceneBook b(4, 256, 1024, 512);
  CHECK(b.set_slot(kSceneDem, 3, kDem) == kSceneOk);
  CHECK(b.set_slot(kSceneDem, 9, kDem) == kSceneOk);
  CHECK(b.set_slot(kSceneCostmap, 4, kCm) == kSceneOk);
  CHECK(b.set_episode_scene(0, 9, 4) == kSceneOk);
  CHECK(b.set_episode_scene(1, 3, -1) == kSceneOk);
  // nobody in use: nothing to mismatch
  CHECK(b.mismatch(kSceneDem, kDemOther) == -1);
  b.mark_set(0);
  CHECK(b.mismatch(kSceneDem, kDem) == -1 && b.mismatch(kSceneCostmap, kCm) == -1);
  CHECK(b.mismatch(kSceneDem, kDemOther) == 9);  // names the slot; episode 1 is not in use
  CHECK(b.mismatch(kSceneCostmap, kCmOther) == 4);
  b.mark_set(1);
  CHECK(b.mismatch(kSceneDem, kDemOther) == 3);  // the lowest
  // one field is enough
  SceneGeom g = kDem;
  g.f2 = 0.2f;
  CHECK(b.mismatch(kSceneDem, g) == 3);
  g = kDem;
  g.n1 = 401;
  CHECK(b.mismatch(kSceneDem, g) == 3);
  // a slot set again under the new geometry matches it
  CHECK(b.set_slot(kSceneDem, 3, kDemOther) == kSceneOk);
  CHECK(b.mismatch(kSceneDem, kDemOther) == 9);
  CHECK(b.mismatch(kSceneDem, kDem) == 3);
  // letting go of the slot ends the complaint
  CHECK(b.set_episode_scene(0, -1, 4) == kSceneOk);
  CHECK(b.mismatch(kSceneDem, kDemOther) == -1);
}

int main() {
  check_blocks();
  check_slots();
  check_table();
  check_geometry();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("batch scene book ok\n");
  return 0;
}
