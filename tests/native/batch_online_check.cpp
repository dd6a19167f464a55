// Host check of the "no log" mode of a batch's task book (csrc/mppi_batch_tasks.h): the book of a
// scored list that keeps no log (mppi_batch_set_tasks_scored, keep_log = 0).  Built with ASan + UBSan by
// tests/test_batch_online_book.py; the header needs no HIP header.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "mppi_batch_tasks.h"

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
static const SceneGeom kCm{400, 0, 20.0f, 0.1f, 0.0f};
static const SceneGeom kCmOther{750, 0, 75.0f, 0.2f, 0.0f};

static TaskSpec spec(int variant, int dem, int cm, int64_t K, int max_steps) {
  TaskSpec t;
  t.variant = variant;
  t.dem = dem;
  t.cm = cm;
  t.K = K;
  t.max_steps = max_steps;
  return t;
}

static BatchSceneBook scene_book() {
  BatchSceneBook b(2, 256, 1024, 512);
  CHECK(b.set_slot(kSceneDem, 3, kDem) == kSceneOk);
  CHECK(b.set_slot(kSceneCostmap, 0, kCm) == kSceneOk);
  return b;
}

static TaskError set(BatchTaskBook& tb, const std::vector<TaskSpec>& list, const BatchSceneBook& book, bool keep_log,
                     int variant_rows = 2, int* bad = nullptr, SceneKind* kind = nullptr) {
  return tb.set(list, variant_rows, book, kDem, kCm, 512, bad, kind, keep_log);
}

// caps the logged book refuses: their sum passes the arena's row limit
static void check_caps() {
  const BatchSceneBook book = scene_book();
  const std::vector<TaskSpec> too_many(600, spec(-1, -1, -1, 0, 2147483647));
  CHECK((int64_t)600 * 2147483647 > BatchTaskBook::kMaxRows);
  BatchTaskBook logged, free_;
  int bad = -1;
  CHECK(set(logged, too_many, book, true, 0, &bad) == kTaskRows && bad > 500);
  CHECK(logged.empty() && logged.keeps_log());
  CHECK(set(free_, too_many, book, false, 0) == kTaskOk);
  CHECK(free_.size() == 600 && !free_.keeps_log() && free_.max_cap() == 2147483647);
  // no base rows, no rows in all
  CHECK(free_.total_rows() == 0);
  for (int i = 0; i < 600; i += 37) CHECK(free_.base(i) == -1);
  // a logged list replaces it and has its rows again; clear() is a logged, empty book
  CHECK(set(free_, {spec(-1, -1, -1, 0, 4), spec(-1, -1, -1, 0, 2)}, book, true) == kTaskOk);
  CHECK(free_.keeps_log() && free_.base(0) == 0 && free_.base(1) == 4 && free_.total_rows() == 6);
  CHECK(set(free_, {spec(-1, -1, -1, 0, 4)}, book, false) == kTaskOk);
  CHECK(!free_.keeps_log() && free_.base(0) == -1 && free_.total_rows() == 0 && free_.max_cap() == 4);
  free_.clear();
  CHECK(free_.empty() && free_.keeps_log() && free_.total_rows() == 0 && free_.max_cap() == 0);
}

// every other rule stands
static void check_rules() {
  const BatchSceneBook book = scene_book();
  BatchTaskBook tb;
  int bad = -1;
  SceneKind kind = kSceneDem;
  CHECK(set(tb, {spec(-1, -1, -1, 0, 4), spec(1, 3, 0, 300, 2)}, book, false) == kTaskOk);
  // a refused list names its first offending task and leaves the book as it was
  CHECK(set(tb, {spec(-1, -1, -1, 0, 1), spec(2, -1, -1, 0, 1)}, book, false, 2, &bad) == kTaskVariant && bad == 1);
  CHECK(set(tb, {spec(-1, -1, 5, 0, 1)}, book, false, 2, &bad, &kind) == kTaskSlotEmpty && bad == 0 &&
        kind == kSceneCostmap);
  CHECK(set(tb, {spec(-1, 256, -1, 0, 1)}, book, false, 2, &bad, &kind) == kTaskSlotRange && kind == kSceneDem);
  CHECK(set(tb, {spec(-1, -1, -1, 513, 1)}, book, false) == kTaskKRange);
  CHECK(set(tb, {spec(-1, -1, -1, 0, 0)}, book, false) == kTaskMaxSteps);
  CHECK(tb.set({spec(-1, -1, 0, 0, 1)}, 2, book, kDem, kCmOther, 512, nullptr, &kind, false) == kTaskSlotGeometry);
  CHECK(tb.size() == 2 && !tb.keeps_log() && tb.task(1).K == 300 && tb.max_cap() == 4);
  // what the kernels and the host ask of a list does not depend on the log
  CHECK(tb.need_variants() && tb.need_scene() && tb.any_costmap());
  CHECK(tb.holder(kSceneDem, 3) == 1 && tb.holder(kSceneCostmap, 0) == 1 && tb.holder(kSceneCostmap, 1) == -1);
  CHECK(tb.variant_beyond(1) == 1 && tb.variant_beyond(2) == -1);
  CHECK(tb.mismatch(kSceneCostmap, book, kCmOther) == 0 && tb.mismatch(kSceneCostmap, book, kCm) == -1);
  const SceneRecord r0 = tb.record(0), r1 = tb.record(1);
  CHECK(r0.dem == -1 && r0.cm == -1 && r0.K == 512 && r0.blocks == 2);
  CHECK(r1.dem == 3 && r1.cm == 0 && r1.K == 300 && r1.blocks == 2);
  bool use[4];
  tb.projections({2, 3}, 2, use);
  CHECK(use[2] && use[3]);
  tb.projections({2, 2}, 2, use);
  CHECK(use[2] && !use[3]);
}

int main() {
  check_caps();
  check_rules();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("batch online book ok\n");
  return 0;
}
