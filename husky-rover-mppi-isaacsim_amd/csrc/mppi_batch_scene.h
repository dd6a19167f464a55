// The bookkeeping of a batch's per-episode scenes and trajectory counts (mppi_batch_set_dem /
// _set_costmap / _set_episode_scene / _set_episode_trajectories), as decisions on
// integers only (no HIP header, so tests/native/batch_scene_check.cpp checks them on the host): which
// slots are live and which episodes hold them, whether a slot still has the context's geometry, an
// episode's leaf blocks, and whether the kernels get a table at all.  A wrong answer here is a
// kernel reading a freed DEM.  The buffers of the slots live in mppi_batch (mppi_capi_batch.cpp).
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

namespace mppi {

// What a slot must share with the context for the launch's scalars (rinv_res, cdiv, the plan) to hold.
// DEM: n0 = rows, n1 = cols, f = x_min, y_min, resolution.  Costmap: n0 = size, f = half_width, resolution.
struct SceneGeom {
  int32_t n0 = 0, n1 = 0;
  float f0 = 0, f1 = 0, f2 = 0;
  bool same(const SceneGeom& o) const { return std::memcmp(this, &o, sizeof(SceneGeom)) == 0; }
};
static_assert(sizeof(SceneGeom) == 20, "SceneGeom has no padding (compared bytewise)");

// One episode's record as the kernels read it (BatchScene of mppi_kernels.h).
struct SceneRecord {
  int32_t dem, cm, K, blocks;
};

enum SceneKind { kSceneDem = 0, kSceneCostmap = 1 };
enum SceneError {
  kSceneOk = 0,
  kSceneSlotRange,  // slot index outside the table
  kSceneSlotEmpty,  // an episode given a slot that is not live
  kSceneSlotHeld,   // freeing a slot an episode holds (`who` = the first holder)
  kSceneEpisode,    // episode index out of range
  kSceneKRange,     // K_e outside [1, context K]
};

class BatchSceneBook {
 public:
  static constexpr int kTraj = 256;  // trajectories per leaf block (PAIR_TRAJ)
  static int blocks_for(int64_t K) { return (int)((K + kTraj - 1) / kTraj); }

  BatchSceneBook() = default;
  BatchSceneBook(int episodes, int dem_slots, int costmap_slots, int64_t context_K)
      : K_(context_K), dem_((size_t)episodes, -1), cm_((size_t)episodes, -1), Ke_((size_t)episodes, 0),
        set_((size_t)episodes, 0) {
    live_[kSceneDem].assign((size_t)dem_slots, 0);
    live_[kSceneCostmap].assign((size_t)costmap_slots, 0);
    geom_[kSceneDem].assign((size_t)dem_slots, SceneGeom{});
    geom_[kSceneCostmap].assign((size_t)costmap_slots, SceneGeom{});
  }

  int episodes() const { return (int)dem_.size(); }
  int slots(SceneKind k) const { return (int)live_[k].size(); }
  bool in_range(SceneKind k, int slot) const { return slot >= 0 && slot < slots(k); }
  bool live(SceneKind k, int slot) const { return in_range(k, slot) && live_[k][(size_t)slot]; }

  // The first episode that holds `slot` (set or not: its index outlives mppi_batch_set_episode), or -1.
  int holder(SceneKind k, int slot) const {
    const std::vector<int32_t>& h = k == kSceneDem ? dem_ : cm_;
    for (size_t e = 0; e < h.size(); ++e)
      if (h[e] == slot) return (int)e;
    return -1;
  }

  // A slot was filled (again: its contents are replaced) with the context's geometry `g`.
  SceneError set_slot(SceneKind k, int slot, const SceneGeom& g) {
    if (!in_range(k, slot)) return kSceneSlotRange;
    live_[k][(size_t)slot] = 1;
    geom_[k][(size_t)slot] = g;
    return kSceneOk;
  }
  // May the slot be freed?  Freeing an empty slot is allowed and changes nothing.
  SceneError free_slot(SceneKind k, int slot, int* who = nullptr) {
    if (!in_range(k, slot)) return kSceneSlotRange;
    const int h = holder(k, slot);
    if (h >= 0) {
      if (who) *who = h;
      return kSceneSlotHeld;
    }
    live_[k][(size_t)slot] = 0;
    return kSceneOk;
  }

  // -1 = the context's.  On an error nothing changes; `bad` receives the offending kind.
  SceneError set_episode_scene(int e, int dem_slot, int cm_slot, SceneKind* bad = nullptr) {
    if (e < 0 || e >= episodes()) return kSceneEpisode;
    const int want[2] = {dem_slot, cm_slot};
    for (int k = 0; k < 2; ++k) {
      if (want[k] == -1) continue;
      if (bad) *bad = (SceneKind)k;
      if (!in_range((SceneKind)k, want[k])) return kSceneSlotRange;
      if (!live_[k][(size_t)want[k]]) return kSceneSlotEmpty;
    }
    dem_[(size_t)e] = dem_slot;
    cm_[(size_t)e] = cm_slot;
    return kSceneOk;
  }
  // 0 = the context's K.
  SceneError set_episode_K(int e, int64_t K) {
    if (e < 0 || e >= episodes()) return kSceneEpisode;
    if (K != 0 && (K < 1 || K > K_)) return kSceneKRange;
    Ke_[(size_t)e] = K;
    return kSceneOk;
  }
  void mark_set(int e) { set_[(size_t)e] = 1; }  // mppi_batch_set_episode: the episode is in use
  // A campaign used the episodes as lanes (mppi_batch_run_tasks): none is in use until it is set
  // again.  Their slots and K_e stay.
  void mark_all_unset() { set_.assign(set_.size(), 0); }
  // Does the live slot hold geometry `g`?  (The task list's slots: mppi_batch_tasks.h.)
  bool slot_has_geometry(SceneKind k, int slot, const SceneGeom& g) const {
    return live(k, slot) && geom_[k][(size_t)slot].same(g);
  }

  bool holds_any(int e) const { return dem_[(size_t)e] >= 0 || cm_[(size_t)e] >= 0 || Ke_[(size_t)e] != 0; }
  // Do the kernels get the table?  Only when an episode in use holds a slot or a K of its own.
  bool need_table() const {
    for (int e = 0; e < episodes(); ++e)
      if (set_[(size_t)e] && holds_any(e)) return true;
    return false;
  }
  bool any_costmap_held() const {
    for (int e = 0; e < episodes(); ++e)
      if (set_[(size_t)e] && cm_[(size_t)e] >= 0) return true;
    return false;
  }
  int dem_of(int e) const { return dem_[(size_t)e]; }
  int costmap_of(int e) const { return cm_[(size_t)e]; }
  int64_t K_of(int e) const { return Ke_[(size_t)e] ? Ke_[(size_t)e] : K_; }

  SceneRecord record(int e) const {
    const int64_t K = K_of(e);
    return SceneRecord{dem_[(size_t)e], cm_[(size_t)e], (int32_t)K, blocks_for(K)};
  }

  // The lowest slot of kind k held by an episode in use whose recorded geometry is not `now` (the
  // context's current one), or -1.
  int mismatch(SceneKind k, const SceneGeom& now) const {
    const std::vector<int32_t>& h = k == kSceneDem ? dem_ : cm_;
    int worst = -1;
    for (size_t e = 0; e < h.size(); ++e) {
      const int s = h[e];
      if (!set_[e] || s < 0 || geom_[k][(size_t)s].same(now)) continue;
      if (worst < 0 || s < worst) worst = s;
    }
    return worst;
  }

 private:
  int64_t K_ = 0;
  std::vector<unsigned char> live_[2];
  std::vector<SceneGeom> geom_[2];
  std::vector<int32_t> dem_, cm_;  // [E] slot or -1
  std::vector<int64_t> Ke_;        // [E] 0: the context's
  std::vector<unsigned char> set_;
};

}  // namespace mppi
