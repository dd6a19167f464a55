// The host side of the hazard costmap (mppi_build_costmap_hazard and its kin), as
// plain float64 arithmetic (no HIP header, so tests/native/hazard_tables_check.cpp checks it on the
// host): the slope limit as a cosine, the two tables that say which costmap cell a DEM cell is
// counted into, the inflation threshold T, how the count kernel is tiled, and the refusals.  The
// device does integer work only with what is formed here.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "mppi.h"

namespace mppi {

// ---- the count kernel's tiling (mppi_costmap.hip costmap_hazard_count_kernel)
constexpr int kHzThreads = 256;                  // threads per workgroup
constexpr int kHzCols = 4 * kHzThreads;          // DEM columns per workgroup: one float4 per thread and row
constexpr int kHzUnroll = 4;                     // rows whose loads are in flight together
constexpr int kHzLdsCounters = 4096;             // int32 counters of a workgroup's costmap window (16 KiB)
constexpr int kHzMaxRows = 32;                   // rows per workgroup at most (one halo row each: 3 % extra reads)

// c = (float)cos(max_slope_deg * pi / 180), formed once in float64: a cell is steep iff !(nz >= c).
inline float hazard_cos(float max_slope_deg) {
  return (float)std::cos((double)max_slope_deg * 3.141592653589793 / 180.0);
}

// floor(v) as a costmap index: -1 for anything outside [0, size) (a NaN included).
inline int32_t hazard_index(double v, int32_t size) {
  const double f = std::floor(v);
  return (f >= 0.0 && f < (double)size) ? (int32_t)f : -1;
}

// The frame is that of the rollout's costmap lookup (_avoid_obstacle: column from x + half_width,
// row from -y + half_width), with the centre of DEM cell (j, i) at
// (x_min + (i + 0.5) res, -y_min - (j + 0.5) res), where the rollout's cell index puts it.
//   ci[i] = floor(((double)x_min + (i + 0.5) (double)res + half_width) / rc)
//   rj[j] = floor((half_width - (-(double)y_min - (j + 0.5) (double)res)) / rc),  rc = 2 half_width / size
inline void hazard_tables(int32_t rows, int32_t cols, float x_min, float y_min, float res, int32_t size,
                          double half_width, std::vector<int32_t>& ci, std::vector<int32_t>& rj) {
  const double rc = 2 * half_width / size;
  ci.resize((size_t)cols);
  rj.resize((size_t)rows);
  for (int32_t i = 0; i < cols; ++i)
    ci[i] = hazard_index(((double)x_min + (i + 0.5) * (double)res + half_width) / rc, size);
  for (int32_t j = 0; j < rows; ++j)
    rj[j] = hazard_index((half_width - (-(double)y_min - (j + 0.5) * (double)res)) / rc, size);
}

// T = floor((inflate / rc)^2) in float64; false when it does not fit int32.
inline bool hazard_threshold(float inflate, int32_t size, double half_width, int32_t* T) {
  const double rc = 2 * half_width / size;
  const double q = (double)inflate / rc;
  const double t = std::floor(q * q);
  if (!(t >= 0.0 && t <= 2147483647.0)) return false;
  *T = (int32_t)t;
  return true;
}

// The refusals of the rule.  Empty string: fine; else the message, naming the field.
inline std::string hazard_check(const mppi_hazard& hz, int32_t size, double half_width) {
  if (!std::isfinite(hz.max_slope_deg) || !(hz.max_slope_deg > 0.0f && hz.max_slope_deg < 90.0f))
    return "hazard: max_slope_deg must be finite and in (0, 90)";
  if (!std::isfinite(hz.inflate) || hz.inflate < 0.0f) return "hazard: inflate must be finite and >= 0";
  if (hz.min_cells < 1) return "hazard: min_cells must be >= 1";
  if (hz.reserved != 0) return "hazard: reserved must be 0";
  if (!std::isfinite(half_width) || !(half_width > 0.0) || size < 1)
    return "hazard: the costmap needs size >= 1 and a finite half_width > 0";
  int32_t T = 0;
  if (!hazard_threshold(hz.inflate, size, half_width, &T))
    return "hazard: inflate: T = floor((inflate / (2 half_width / size))^2) does not fit int32";
  return std::string();
}

// Rows per workgroup of the count kernel, and whether its costmap window fits the LDS counters.
// A workgroup covers kHzCols DEM columns and R rows, i.e. at most ceil(n res / rc) + 1 costmap
// columns / rows.  R is the largest of 32, 16, 8 whose window fits and that still gives 512
// workgroups (two per compute unit), else the smallest of them that fits.  The 512 and the row
// counts are choices, not measured: at both profiled scenes the counters admit one
// candidate only, 8 rows at 1500^2 / 750^2 and 32 at 8192^2 / 1024^2.  When not even kHzUnroll rows fit (a costmap finer than the DEM, where
// a costmap cell gets one DEM cell at most and there is nothing to reduce), lds = false: the
// workgroup adds its steep cells to the count plane directly.
struct HazardTiling {
  int rows_per_group;
  bool lds;
};
inline HazardTiling hazard_tiling(int32_t rows, int32_t cols, float res, int32_t size, double half_width) {
  const double ratio = (double)res / (2 * half_width / size);  // costmap cells per DEM cell
  auto span = [&](int n) { return std::ceil(n * ratio) + 1.0; };
  const int64_t tiles = ((int64_t)cols + kHzCols - 1) / kHzCols;
  const double wi = span(cols < kHzCols ? cols : kHzCols);
  int fit = 0;
  for (int R = kHzMaxRows; R >= kHzUnroll; R /= 2) {
    if (!(wi * span(R) <= (double)kHzLdsCounters)) continue;
    if (!fit) fit = R;
    if (R >= 8 && tiles * (((int64_t)rows + R - 1) / R) >= 512) return HazardTiling{R, true};
  }
  if (!fit) return HazardTiling{8, false};
  return HazardTiling{fit < 8 ? fit : 8, true};
}

}  // namespace mppi
