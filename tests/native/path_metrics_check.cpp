// Host check of csrc/mppi_path_metrics.h (compute_path_metrics of the reference on executed paths) and of
// dm_atan2 (csrc/mppi_detmath.h).  Built with ASan + UBSan and -ffp-contract=off by
// tests/test_path_metrics_cpu.py; neither header needs a HIP header on the host.
//  * the online form (metrics_row, one row at a time, as the advance lane and the tracked ingest feed
//    it) equals the whole-path form (path_metrics_rows, as the log scorer calls it) bit for bit, for
//    every path length 0 .. 70, on a path with a repeated pose and a level stretch; a second path fed
//    into the same state right after shows that row 0 starts over;
//  * prints dm_atan2 on a fixed set of points and the metrics of the 70-row path as hex floats, which
//    the test compares with the numpy restatement (mppi_amd/batch.py) bit for bit.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "mppi_path_metrics.h"

using namespace mppi;

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static uint32_t g_rng = 12345u;
static double uniform() {  // LCG, [0, 1)
  g_rng = g_rng * 1664525u + 1013904223u;
  return (double)(g_rng >> 8) / 16777216.0;
}

static bool same(const PathMetrics& a, const PathMetrics& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

// [L][8] log rows: a walk that climbs and descends, rows 24 .. 27 one repeated pose, rows 40 .. 61 level
static std::vector<float> make_path(int L) {
  std::vector<float> rows((size_t)L * 8, 0.0f);
  double x = -3.0, y = 2.0, z = 1.0;
  for (int i = 0; i < L; ++i) {
    if (i < 24 || i > 27) {
      x += 0.09 * (uniform() - 0.3);
      y += 0.09 * (uniform() - 0.5);
      if (i < 40 || i > 61) z += 0.02 * (uniform() - (i < 30 ? 0.2 : 0.7));
    }
    rows[(size_t)i * 8] = (float)x;
    rows[(size_t)i * 8 + 1] = (float)y;
    rows[(size_t)i * 8 + 2] = (float)z;
    rows[(size_t)i * 8 + 6] = 1.0f;  // (the other columns are not read)
  }
  return rows;
}

static void check_online() {
  const std::vector<float> rows = make_path(70);
  PathMetricsAcc acc;
  std::memset(&acc, 0xff, sizeof(acc));  // whatever the lane's record held: row 0 starts over
  for (int L = 0; L <= 70; ++L) {
    const PathMetrics whole = path_metrics_rows(rows.data(), 8, L);
    PathMetrics online{0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < L; ++r) {
      metrics_row(acc, r, rows[(size_t)r * 8], rows[(size_t)r * 8 + 1], rows[(size_t)r * 8 + 2]);
      online = acc.m;
    }
    CHECK(same(whole, online));
    if (L < 22) CHECK(whole.length20 == 0.0 && whole.angle_up == 0.0 && whole.angle_down == 0.0 && whole.distance_up == 0.0);
    if (L == 22 || L == 42 || L == 62) CHECK(whole.length20 > path_metrics_rows(rows.data(), 8, L - 1).length20);
    if (L == 23 || L == 43 || L == 63) CHECK(same(whole, path_metrics_rows(rows.data(), 8, L - 1)));
  }
  const PathMetrics all = path_metrics_rows(rows.data(), 8, 70);
  CHECK(all.angle_up > 0.0 && all.angle_down > 0.0 && all.distance_up > 0.0);
  // rows of 3 floats (a caller's [L][3] path) give the same
  std::vector<float> xyz(70 * 3);
  for (int r = 0; r < 70; ++r)
    for (int k = 0; k < 3; ++k) xyz[(size_t)r * 3 + k] = rows[(size_t)r * 8 + k];
  CHECK(same(all, path_metrics_rows(xyz.data(), 3, 70)));
  for (int r = 0; r < 70; ++r) std::printf("row %a %a %a\n", (double)xyz[r * 3], (double)xyz[r * 3 + 1], (double)xyz[r * 3 + 2]);
  std::printf("metrics %a %a %a %a\n", all.length20, all.angle_up, all.angle_down, all.distance_up);
}

// a zero-length segment adds nothing; a level one adds |0| to angle_down and nothing to distance_up
static void check_segments() {
  PathMetrics m{0.0, 0.0, 0.0, 0.0};
  const float a[3] = {1.5f, -2.0f, 0.25f};
  metrics_segment(m, a, 1.5f, -2.0f, 0.25f);
  CHECK(m.length20 == 0.0 && m.angle_up == 0.0 && m.angle_down == 0.0 && m.distance_up == 0.0);
  metrics_segment(m, a, 4.5f, 2.0f, 0.25f);
  CHECK(m.length20 == 5.0 && m.angle_up == 0.0 && m.angle_down == 0.0 && m.distance_up == 0.0);
  metrics_segment(m, a, 1.5f, -2.0f, 1.25f);  // straight up: 90 degrees
  CHECK(m.length20 == 6.0 && m.angle_up == 90.0 && m.distance_up == 1.0);
  metrics_segment(m, a, 2.5f, -2.0f, -0.75f);  // 45 degrees down
  CHECK(m.angle_down > 44.99999999 && m.angle_down < 45.00000001 && m.distance_up == 1.0);
}

static void print_atan2() {
  const double special[] = {0.0, 1.0, -1.0, 0.5, -0.5, 2.0, -2.0, 1e-300, -1e-300, 1e300, -1e300, 3.0, 1e-8, -7.25};
  const int n = (int)(sizeof(special) / sizeof(special[0]));
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j) std::printf("atan2 %a %a %a\n", special[i], special[j], dm_atan2(special[i], special[j]));
  for (int i = 0; i < 1200; ++i) {
    const double y = (uniform() - 0.5) * 20.0, x = (uniform() - 0.5) * (i % 3 ? 20.0 : 0.02);
    std::printf("atan2 %a %a %a\n", y, x, dm_atan2(y, x));
  }
  CHECK(dm_atan2(0.0, 0.0) == 0.0);
  CHECK(dm_atan2(1.0, 0.0) == 1.5707963267948966);
  CHECK(dm_atan2(0.0, -1.0) == 3.141592653589793);
}

int main() {
  check_online();
  check_segments();
  print_atan2();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("path metrics ok\n");
  return 0;
}
