// compute_path_metrics of the reference (MPPI_isaac.py:231-256, k = 20) on an executed path, in float64:
// what the 2D-vs-3D comparison quotes per run (path length, summed climb and descent angles, metres
// climbed; the raw columns of old_files/stats.py).  One statement of the segment rule and of the small
// state that feeds it one row at a time, as plain arithmetic (no HIP header, so
// tests/native/path_metrics_check.cpp walks it on the host): the log scorer's metrics kernel
// (mppi_score.hip) calls the whole-path form, the advance lane of a scored list and the tracked ingest
// (mppi_batch_kernels.h) the online form.  Every operation is IEEE float64 under -ffp-contract=off and
// the sums run in row order, so the three agree bit for bit with each other and with
// mppi_amd.batch.path_metrics.
//
// Waypoints are the rows' float32 (x, y, z) widened.  Segments m = 0, 1, ...: s = p[20 m + 21] - p[20 m]
// while 20 m + 21 < L (the reference's i = 1, 21, ... < L - 20 with p[i + 20] - p[i - 1]; consecutive
// segments overlap by one row, which is the reference's).  Per segment hh = s.x s.x + s.y s.y,
// n = sqrt(hh + s.z s.z), length20 += n; if n > 0: a = dm_atan2(s.z, sqrt(hh)) (180 / pi), a > 0 adds a
// to angle_up, else |a| to angle_down; if s.z > 0: distance_up += s.z.  Fewer than 22 rows: zeros.
#pragma once

#include "mppi_detmath.h"

namespace mppi {

constexpr int kMetricsStride = 20;  // the reference's k

struct PathMetrics {  // mppi_path_metrics (include/mppi.h) field for field
  double length20, angle_up, angle_down, distance_up;
};
static_assert(sizeof(PathMetrics) == 32, "PathMetrics layout");

// One segment from anchor a (row 20 m) to p (row 20 m + 21) enters the sums.
MPPI_HD void metrics_segment(PathMetrics& m, const float (&a)[3], float px, float py, float pz) {
  const double sx = (double)px - (double)a[0], sy = (double)py - (double)a[1], sz = (double)pz - (double)a[2];
  const double hh = sx * sx + sy * sy;
  const double n = __builtin_sqrt(hh + sz * sz);
  m.length20 = m.length20 + n;
  if (n > 0.0) {
    const double ang = dm_atan2(sz, __builtin_sqrt(hh)) * 57.29577951308232;  // 180 / pi (np.degrees)
    if (ang > 0.0)
      m.angle_up = m.angle_up + ang;
    else
      m.angle_down = m.angle_down + (ang < 0.0 ? -ang : ang);
  }
  if (sz > 0.0) m.distance_up = m.distance_up + sz;
}

// The whole-path form: L rows of `stride` floats each, x, y, z first.
MPPI_HD PathMetrics path_metrics_rows(const float* rows, int stride, int L) {
  PathMetrics m{0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i + kMetricsStride + 1 < L; i += kMetricsStride) {
    const float* a = rows + (size_t)i * stride;
    const float* p = rows + (size_t)(i + kMetricsStride + 1) * stride;
    const float anchor[3] = {a[0], a[1], a[2]};
    metrics_segment(m, anchor, p[0], p[1], p[2]);
  }
  return m;
}

// The online form: two pending anchors (rows 20 m and 20 (m + 1)); the segment of anchor 20 m enters
// when row 20 m + 21 arrives, and by then row 20 (m + 1) has passed.  Row 0 starts the path over.
struct PathMetricsAcc {
  float a0[3], a1[3];
  PathMetrics m;
};
static_assert(sizeof(PathMetricsAcc) == 56, "PathMetricsAcc layout");

MPPI_HD void metrics_row(PathMetricsAcc& s, int row, float x, float y, float z) {
  const int k = row % kMetricsStride;
  if (row == 0) {
    s.m = PathMetrics{0.0, 0.0, 0.0, 0.0};
    s.a0[0] = x;
    s.a0[1] = y;
    s.a0[2] = z;
  } else if (k == 0) {
    s.a1[0] = x;
    s.a1[1] = y;
    s.a1[2] = z;
  } else if (k == 1 && row > kMetricsStride) {
    metrics_segment(s.m, s.a0, x, y, z);
    s.a0[0] = s.a1[0];
    s.a0[1] = s.a1[1];
    s.a0[2] = s.a1[2];
  }
}

}  // namespace mppi
