// The bookkeeping of a batch's task list (mppi_batch_set_tasks / _run_tasks), as
// decisions on integers only (no HIP header, so tests/native/batch_tasks_check.cpp walks them on the
// host): whether a task may be listed, each task's first row of the log arena, which projections,
// slots and variant rows the list uses, whether the kernels need the variant and the scene table, and
// what may be freed while the list stands.  A wrong answer here is a lane writing its log over
// another task's rows, or a kernel reading a freed DEM.  Beside mppi_batch_scene.h, whose book knows
// the slots.
#pragma once
#include <cstdint>
#include <vector>

#include "mppi_batch_scene.h"

namespace mppi {

// The integer part of one mppi_batch_task.
struct TaskSpec {
  int32_t variant = -1;          // row of the variant table, -1: none
  int32_t dem = -1, cm = -1;     // slots, -1: the context's
  int64_t K = 0;                 // 0: the context's
  int32_t max_steps = 1;
};

enum TaskError {
  kTaskOk = 0,
  kTaskVariant,       // variant index outside [-1, rows of the table)
  kTaskSlotRange,     // a slot index outside [-1, slots)         (`kind` says which)
  kTaskSlotEmpty,     // a slot that is not live
  kTaskSlotGeometry,  // a live slot set under another geometry than the context's current one
  kTaskKRange,        // K outside [1, context K] (0: the context's)
  kTaskMaxSteps,      // max_steps < 1
  kTaskRows,          // the caps sum to more rows than the arena may have (a list that keeps a log)
};

class BatchTaskBook {
 public:
  static constexpr int64_t kMaxRows = (int64_t)1 << 40;  // rows of 32 bytes: far beyond any device

  int size() const { return (int)t_.size(); }
  bool empty() const { return t_.empty(); }
  void clear() {
    t_.clear();
    base_.clear();
    total_ = 0;
    max_cap_ = 0;
    keep_log_ = true;
  }

  // May `t` be listed?  The rules of the per-episode setters (BatchSceneBook::set_episode_scene /
  // set_episode_K, mppi_batch_set_episode_variant), and a slot must have the context's geometry now.
  static TaskError check(const TaskSpec& t, int variant_rows, const BatchSceneBook& book, const SceneGeom& dem_now,
                         const SceneGeom& cm_now, int64_t context_K, SceneKind* kind = nullptr) {
    if (t.variant < -1 || t.variant >= variant_rows) return kTaskVariant;
    const int want[2] = {t.dem, t.cm};
    for (int k = 0; k < 2; ++k) {
      if (want[k] == -1) continue;
      if (kind) *kind = (SceneKind)k;
      if (!book.in_range((SceneKind)k, want[k])) return kTaskSlotRange;
      if (!book.live((SceneKind)k, want[k])) return kTaskSlotEmpty;
      if (!book.slot_has_geometry((SceneKind)k, want[k], k == kSceneDem ? dem_now : cm_now)) return kTaskSlotGeometry;
    }
    if (t.K != 0 && (t.K < 1 || t.K > context_K)) return kTaskKRange;
    if (t.max_steps < 1) return kTaskMaxSteps;
    return kTaskOk;
  }

  // Replace the list.  On an error nothing changes; `bad` receives the first offending task.
  // keep_log false (a scored list that keeps no log, mppi_batch_set_tasks_scored): there is no arena, so
  // no task has base rows and the caps' sum has no limit; every other rule stands.
  TaskError set(const std::vector<TaskSpec>& tasks, int variant_rows, const BatchSceneBook& book,
                const SceneGeom& dem_now, const SceneGeom& cm_now, int64_t context_K, int* bad = nullptr,
                SceneKind* kind = nullptr, bool keep_log = true) {
    std::vector<int64_t> base(keep_log ? tasks.size() : 0);
    int64_t rows = 0;
    int cap = 0;
    for (size_t i = 0; i < tasks.size(); ++i) {
      if (bad) *bad = (int)i;
      const TaskError err = check(tasks[i], variant_rows, book, dem_now, cm_now, context_K, kind);
      if (err != kTaskOk) return err;
      if (tasks[i].max_steps > cap) cap = tasks[i].max_steps;
      if (!keep_log) continue;
      base[i] = rows;
      rows += tasks[i].max_steps;
      if (rows > kMaxRows) return kTaskRows;
    }
    t_ = tasks;
    base_.swap(base);
    total_ = rows;
    max_cap_ = cap;
    K_ = context_K;
    keep_log_ = keep_log;
    return kTaskOk;
  }

  const TaskSpec& task(int i) const { return t_[(size_t)i]; }
  // Task i's rows of the arena are [base(i), base(i) + max_steps): the prefix sum of the caps before it.
  // A list that keeps no log hands out no base rows: -1, and no rows in all.
  int64_t base(int i) const { return keep_log_ ? base_[(size_t)i] : -1; }
  bool keeps_log() const { return keep_log_; }
  int64_t total_rows() const { return total_; }
  int max_cap() const { return max_cap_; }

  // The scene record a lane runs task i with (BatchScene of mppi_kernels.h).
  SceneRecord record(int i) const {
    const TaskSpec& t = t_[(size_t)i];
    const int64_t K = t.K ? t.K : K_;
    return SceneRecord{t.dem, t.cm, (int32_t)K, BatchSceneBook::blocks_for(K)};
  }

  // Do the kernels of a campaign get the variant table / the scene table?
  bool need_variants() const {
    for (const TaskSpec& t : t_)
      if (t.variant >= 0) return true;
    return false;
  }
  bool need_scene() const {
    for (const TaskSpec& t : t_)
      if (t.dem >= 0 || t.cm >= 0 || t.K != 0) return true;
    return false;
  }
  bool any_costmap() const {
    for (const TaskSpec& t : t_)
      if (t.cm >= 0) return true;
    return false;
  }

  // The projections (2 / 3) the list uses: a task's variant's (variant_proj[row]), or `run_proj` for a
  // task without one.  use[2], use[3].
  void projections(const std::vector<int>& variant_proj, int run_proj, bool use[4]) const {
    use[0] = use[1] = use[2] = use[3] = false;
    for (const TaskSpec& t : t_) {
      const int pj = t.variant >= 0 ? variant_proj[(size_t)t.variant] : run_proj;
      if (pj >= 0 && pj < 4) use[pj] = true;
    }
  }

  // What the list holds while it stands: the first task on `slot` (or -1), and the first task whose
  // variant row a table of `rows` rows would no longer have (or -1).
  int holder(SceneKind k, int slot) const {
    for (size_t i = 0; i < t_.size(); ++i)
      if ((k == kSceneDem ? t_[i].dem : t_[i].cm) == slot) return (int)i;
    return -1;
  }
  int variant_beyond(int rows) const {
    for (size_t i = 0; i < t_.size(); ++i)
      if (t_[i].variant >= rows) return (int)i;
    return -1;
  }
  // The lowest slot of kind k a listed task holds whose geometry is not `now` (any more), or -1.
  int mismatch(SceneKind k, const BatchSceneBook& book, const SceneGeom& now) const {
    int worst = -1;
    for (const TaskSpec& t : t_) {
      const int s = k == kSceneDem ? t.dem : t.cm;
      if (s < 0 || book.slot_has_geometry(k, s, now)) continue;
      if (worst < 0 || s < worst) worst = s;
    }
    return worst;
  }

 private:
  std::vector<TaskSpec> t_;
  std::vector<int64_t> base_;
  int64_t total_ = 0, K_ = 0;
  int max_cap_ = 0;
  bool keep_log_ = true;
};

// The batch steps the claim rule needs for tasks of the given lengths on `lanes` lanes: greedy list
// scheduling in list order; a task of length 0 is consumed without a step (mppi_amd.batch
// campaign_makespan is the same rule in Python).
inline int64_t campaign_makespan(const std::vector<int64_t>& lengths, int lanes) {
  std::vector<int64_t> busy;  // steps left of each running lane
  size_t next = 0;
  int64_t steps = 0;
  auto fill = [&]() {
    while ((int)busy.size() < lanes && next < lengths.size()) {
      const int64_t n = lengths[next++];
      if (n > 0) busy.push_back(n);
    }
  };
  fill();
  while (!busy.empty()) {
    ++steps;
    for (size_t i = 0; i < busy.size();) {
      if (--busy[i] == 0) {
        busy[i] = busy.back();
        busy.pop_back();
      } else {
        ++i;
      }
    }
    fill();
  }
  return steps;
}

}  // namespace mppi
