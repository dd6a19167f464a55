// Host check of the bookkeeping of a batch's task list (csrc/mppi_batch_tasks.h).  Built with ASan +
// UBSan by tests/test_batch_tasks_book.py; the header needs no HIP header.
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
static const SceneGeom kDemOther{1500, 1500, -75.0f, -75.0f, 0.1f};
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
  CHECK(b.set_slot(kSceneDem, 255, kDem) == kSceneOk);
  CHECK(b.set_slot(kSceneCostmap, 0, kCm) == kSceneOk);
  CHECK(b.set_slot(kSceneCostmap, 1023, kCm) == kSceneOk);
  return b;
}

static void check_refusals() {
  const BatchSceneBook book = scene_book();
  SceneKind kind = kSceneCostmap;
  auto chk = [&](const TaskSpec& t, SceneKind* k = nullptr) { return BatchTaskBook::check(t, 2, book, kDem, kCm, 512, k); };
  CHECK(chk(spec(-1, -1, -1, 0, 1)) == kTaskOk);
  CHECK(chk(spec(1, 3, 1023, 512, 3500)) == kTaskOk);
  CHECK(chk(spec(2, -1, -1, 0, 1)) == kTaskVariant);
  CHECK(chk(spec(-2, -1, -1, 0, 1)) == kTaskVariant);
  CHECK(chk(spec(-1, 256, -1, 0, 1), &kind) == kTaskSlotRange && kind == kSceneDem);
  CHECK(chk(spec(-1, -2, -1, 0, 1), &kind) == kTaskSlotRange && kind == kSceneDem);
  CHECK(chk(spec(-1, 3, 1024, 0, 1), &kind) == kTaskSlotRange && kind == kSceneCostmap);
  CHECK(chk(spec(-1, 4, -1, 0, 1), &kind) == kTaskSlotEmpty && kind == kSceneDem);
  CHECK(chk(spec(-1, 3, 7, 0, 1), &kind) == kTaskSlotEmpty && kind == kSceneCostmap);
  CHECK(chk(spec(-1, -1, -1, 513, 1)) == kTaskKRange);
  CHECK(chk(spec(-1, -1, -1, -1, 1)) == kTaskKRange);
  CHECK(chk(spec(-1, -1, -1, (int64_t)1 << 40, 1)) == kTaskKRange);
  CHECK(chk(spec(-1, -1, -1, 1, 1)) == kTaskOk);
  CHECK(chk(spec(-1, -1, -1, 0, 0)) == kTaskMaxSteps);
  CHECK(chk(spec(-1, -1, -1, 0, -5)) == kTaskMaxSteps);
  // a slot set under another geometry than the context's current one
  CHECK(BatchTaskBook::check(spec(-1, 3, -1, 0, 1), 2, book, kDemOther, kCm, 512, &kind) == kTaskSlotGeometry &&
        kind == kSceneDem);
  CHECK(BatchTaskBook::check(spec(-1, -1, 0, 0, 1), 2, book, kDem, kCmOther, 512, &kind) == kTaskSlotGeometry &&
        kind == kSceneCostmap);
  // without a table no task may name a row
  CHECK(BatchTaskBook::check(spec(0, -1, -1, 0, 1), 0, book, kDem, kCm, 512) == kTaskVariant);

  // set: the first offending task is named and the list stays as it was
  BatchTaskBook tb;
  int bad = -1;
  CHECK(tb.set({spec(-1, -1, -1, 0, 4), spec(0, 3, -1, 300, 2)}, 2, book, kDem, kCm, 512, &bad) == kTaskOk);
  CHECK(tb.size() == 2 && tb.total_rows() == 6);
  CHECK(tb.set({spec(-1, -1, -1, 0, 4), spec(-1, -1, -1, 0, 9), spec(-1, -1, 5, 0, 1), spec(9, -1, -1, 0, 1)}, 2, book,
               kDem, kCm, 512, &bad, &kind) == kTaskSlotEmpty);
  CHECK(bad == 2 && kind == kSceneCostmap);
  CHECK(tb.size() == 2 && tb.total_rows() == 6 && tb.task(1).K == 300);
}

static void check_rows() {
  const BatchSceneBook book = scene_book();
  BatchTaskBook tb;
  CHECK(tb.empty() && tb.total_rows() == 0 && tb.max_cap() == 0);
  const int caps[6] = {3, 1, 3500, 2, 13, 1};
  std::vector<TaskSpec> list;
  for (int c : caps) list.push_back(spec(-1, -1, -1, 0, c));
  CHECK(tb.set(list, 0, book, kDem, kCm, 512) == kTaskOk);
  int64_t want = 0;
  for (int i = 0; i < 6; ++i) {  // disjoint, gapless, in list order
    CHECK(tb.base(i) == want);
    want += caps[i];
  }
  CHECK(tb.total_rows() == want && tb.max_cap() == 3500);
  // 2 000 tasks of 3 500 steps: 7 000 000 rows, past nothing in 64 bits; the last task's rows end at the total
  std::vector<TaskSpec> big(2000, spec(-1, -1, -1, 0, 3500));
  CHECK(tb.set(big, 0, book, kDem, kCm, 512) == kTaskOk);
  CHECK(tb.base(1999) + 3500 == tb.total_rows() && tb.total_rows() == (int64_t)7000000);
  // rows past 2^31 stay exact
  std::vector<TaskSpec> huge(3, spec(-1, -1, -1, 0, 2147483647));
  CHECK(tb.set(huge, 0, book, kDem, kCm, 512) == kTaskOk);
  CHECK(tb.base(2) == (int64_t)2 * 2147483647 && tb.total_rows() == (int64_t)3 * 2147483647);
  std::vector<TaskSpec> too_many(600, spec(-1, -1, -1, 0, 2147483647));
  int bad = -1;
  CHECK(tb.set(too_many, 0, book, kDem, kCm, 512, &bad) == kTaskRows && bad > 500);
  CHECK(tb.size() == 3);
  tb.clear();
  CHECK(tb.empty() && tb.total_rows() == 0 && tb.holder(kSceneDem, 3) == -1 && tb.variant_beyond(0) == -1);
}

static void check_records_and_tables() {
  const BatchSceneBook book = scene_book();
  BatchTaskBook tb;
  CHECK(tb.set({spec(-1, -1, -1, 0, 1), spec(-1, -1, -1, 0, 2)}, 3, book, kDem, kCm, 512) == kTaskOk);
  CHECK(!tb.need_variants() && !tb.need_scene() && !tb.any_costmap());
  SceneRecord r = tb.record(0);
  CHECK(r.dem == -1 && r.cm == -1 && r.K == 512 && r.blocks == 2);
  const int64_t ks[5] = {1, 256, 257, 300, 512};
  const int blocks[5] = {1, 1, 2, 2, 2};
  std::vector<TaskSpec> list;
  for (int64_t k : ks) list.push_back(spec(-1, -1, -1, k, 1));
  CHECK(tb.set(list, 3, book, kDem, kCm, 512) == kTaskOk);
  CHECK(tb.need_scene() && !tb.need_variants() && !tb.any_costmap());  // a K of its own needs the table
  for (int i = 0; i < 5; ++i) CHECK(tb.record(i).K == (int32_t)ks[i] && tb.record(i).blocks == blocks[i]);
  CHECK(tb.set({spec(-1, -1, -1, 0, 1), spec(2, -1, -1, 0, 1)}, 3, book, kDem, kCm, 512) == kTaskOk);
  CHECK(tb.need_variants() && !tb.need_scene());
  CHECK(tb.set({spec(-1, -1, -1, 0, 1), spec(-1, -1, 1023, 0, 1), spec(-1, 255, -1, 0, 1)}, 3, book, kDem, kCm, 512) ==
        kTaskOk);
  CHECK(tb.need_scene() && tb.any_costmap());
  r = tb.record(1);
  CHECK(r.dem == -1 && r.cm == 1023 && r.K == 512 && r.blocks == 2);
  CHECK(tb.record(2).dem == 255);
}

static void check_projections() {
  const BatchSceneBook book = scene_book();
  BatchTaskBook tb;
  const std::vector<int> vproj = {2, 3, 2};
  bool use[4];
  CHECK(tb.set({spec(-1, -1, -1, 0, 1), spec(-1, -1, -1, 0, 1)}, 3, book, kDem, kCm, 512) == kTaskOk);
  tb.projections(vproj, 3, use);
  CHECK(!use[0] && !use[1] && !use[2] && use[3]);
  tb.projections(vproj, 2, use);
  CHECK(use[2] && !use[3]);
  CHECK(tb.set({spec(1, -1, -1, 0, 1), spec(1, -1, -1, 0, 1)}, 3, book, kDem, kCm, 512) == kTaskOk);
  tb.projections(vproj, 2, use);  // every task has a variant: the run's projection is not launched
  CHECK(!use[2] && use[3]);
  CHECK(tb.set({spec(0, -1, -1, 0, 1), spec(-1, -1, -1, 0, 1), spec(2, -1, -1, 0, 1)}, 3, book, kDem, kCm, 512) == kTaskOk);
  tb.projections(vproj, 3, use);
  CHECK(use[2] && use[3]);
  tb.projections(vproj, 2, use);
  CHECK(use[2] && !use[3]);
  tb.clear();
  tb.projections(vproj, 3, use);
  CHECK(!use[2] && !use[3]);
}

static void check_holds() {
  BatchSceneBook book = scene_book();
  BatchTaskBook tb;
  CHECK(tb.set({spec(-1, -1, -1, 0, 1), spec(1, 3, -1, 0, 1), spec(0, 3, 1023, 0, 1), spec(-1, -1, 0, 0, 1)}, 2, book,
               kDem, kCm, 512) == kTaskOk);
  CHECK(tb.holder(kSceneDem, 3) == 1 && tb.holder(kSceneCostmap, 1023) == 2 && tb.holder(kSceneCostmap, 0) == 3);
  CHECK(tb.holder(kSceneDem, 255) == -1 && tb.holder(kSceneCostmap, 3) == -1);
  CHECK(tb.variant_beyond(2) == -1 && tb.variant_beyond(1) == 1 && tb.variant_beyond(0) == 1);
  // the context's geometry changes under the list: the lowest held slot is named
  CHECK(tb.mismatch(kSceneDem, book, kDem) == -1 && tb.mismatch(kSceneCostmap, book, kCm) == -1);
  CHECK(tb.mismatch(kSceneDem, book, kDemOther) == 3);
  CHECK(tb.mismatch(kSceneCostmap, book, kCmOther) == 0);
  CHECK(book.set_slot(kSceneCostmap, 0, kCmOther) == kSceneOk);  // set again under the new geometry
  CHECK(tb.mismatch(kSceneCostmap, book, kCmOther) == 1023);
  // once the list is replaced the slots are free again
  CHECK(tb.set({spec(-1, -1, -1, 0, 1)}, 2, book, kDem, kCm, 512) == kTaskOk);
  CHECK(tb.holder(kSceneDem, 3) == -1 && tb.variant_beyond(0) == -1);
}

static void check_unset() {
  BatchSceneBook book = scene_book();
  CHECK(book.set_episode_scene(0, 3, -1) == kSceneOk);
  book.mark_set(0);
  book.mark_set(1);
  CHECK(book.need_table() && book.mismatch(kSceneDem, kDemOther) == 3);
  book.mark_all_unset();  // a campaign used the episodes as lanes
  CHECK(!book.need_table() && book.mismatch(kSceneDem, kDemOther) == -1);
  CHECK(book.dem_of(0) == 3 && book.holder(kSceneDem, 3) == 0);  // the episode's slot outlives it
  book.mark_set(0);
  CHECK(book.need_table());
  CHECK(book.slot_has_geometry(kSceneDem, 3, kDem) && !book.slot_has_geometry(kSceneDem, 3, kDemOther));
  CHECK(!book.slot_has_geometry(kSceneDem, 4, kDem) && !book.slot_has_geometry(kSceneDem, 256, kDem));
}

// Brute force: every lane explicitly, one batch step at a time.
static int64_t simulate(const std::vector<int64_t>& len, int lanes) {
  std::vector<int64_t> left((size_t)lanes, 0);
  std::vector<char> on((size_t)lanes, 0);
  size_t next = 0;
  auto claim = [&](int l) {
    on[(size_t)l] = 0;
    while (next < len.size()) {
      const int64_t n = len[next++];
      if (n == 0) continue;
      left[(size_t)l] = n;
      on[(size_t)l] = 1;
      return;
    }
  };
  for (int l = 0; l < lanes; ++l) claim(l);
  int64_t steps = 0;
  for (;;) {
    bool any = false;
    for (int l = 0; l < lanes; ++l) any = any || on[(size_t)l];
    if (!any) return steps;
    ++steps;
    for (int l = 0; l < lanes; ++l)
      if (on[(size_t)l] && --left[(size_t)l] == 0) claim(l);
  }
}

static void check_makespan() {
  CHECK(campaign_makespan({3, 9, 2, 2, 4}, 2) == 11);
  CHECK(campaign_makespan({}, 4) == 0 && campaign_makespan({0, 0}, 1) == 0);
  CHECK(campaign_makespan({5}, 64) == 5 && campaign_makespan({1, 2, 3}, 1) == 6);
  uint32_t s = 12345u;
  auto rnd = [&]() {
    s = s * 1664525u + 1013904223u;
    return (int)(s >> 16);
  };
  for (int it = 0; it < 300; ++it) {
    std::vector<int64_t> len((size_t)(rnd() % 12));
    for (int64_t& n : len) n = rnd() % 3 == 0 ? 0 : rnd() % 9;
    const int lanes = 1 + rnd() % 6;
    CHECK(campaign_makespan(len, lanes) == simulate(len, lanes));
  }
}

int main() {
  check_refusals();
  check_rows();
  check_records_and_tables();
  check_projections();
  check_holds();
  check_unset();
  check_makespan();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("batch task book ok\n");
  return 0;
}
