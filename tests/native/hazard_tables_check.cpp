// Host check of the hazard costmap's host side (csrc/mppi_hazard.h): the two cell tables for DEMs
// inside, straddling and outside the costmap, the inflation threshold T, the slope cosine, the count
// kernel's tiling and every refusal.  Built with ASan + UBSan by tests/test_hazard_host.py; the header
// needs no HIP header.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mppi_hazard.h"

using namespace mppi;

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

// the tables of a DEM, with the invariants every table has: entries in [-1, size), non-decreasing over
// the entries that are inside, the inside entries one contiguous run
static void tables(int rows, int cols, float x_min, float y_min, float res, int size, double hw,
                   std::vector<int32_t>& ci, std::vector<int32_t>& rj) {
  hazard_tables(rows, cols, x_min, y_min, res, size, hw, ci, rj);  // (exactly sized: ASan sees an overrun)
  CHECK((int)ci.size() == cols && (int)rj.size() == rows);
  for (const std::vector<int32_t>* t : {&ci, &rj}) {
    int prev = -1, runs = 0;
    bool in = false;
    for (int32_t v : *t) {
      CHECK(v >= -1 && v < size);
      if (v >= 0) {
        CHECK(v >= prev);
        prev = v;
        if (!in) ++runs;
      }
      in = v >= 0;
    }
    CHECK(runs <= 1);
  }
}

static void check_tables() {
  std::vector<int32_t> ci, rj;
  // inside, commensurate: 192 cells of 0.78125 m over [-75, 75), 24 costmap cells of 6.25 m: 8 per cell
  tables(192, 192, -75.0f, -75.0f, 150.0f / 192, 24, 75.0, ci, rj);
  for (int i = 0; i < 192; ++i) CHECK(ci[i] == i / 8 && rj[i] == i / 8);
  // a 2 x 2 DEM over the same extent: cell centres at -37.5 and 37.5
  tables(2, 2, -75.0f, -75.0f, 75.0f, 24, 75.0, ci, rj);
  CHECK(ci[0] == 6 && ci[1] == 18 && rj[0] == 6 && rj[1] == 18);
  // the row table runs with -y: row 0 is the top of the map (y = -y_min), which is costmap row 0 only
  // when -y_min = half_width
  tables(4, 4, 0.0f, -10.0f, 1.0f, 20, 10.0, ci, rj);  // x in [0, 4), y in (6, 10]
  CHECK(ci[0] == 10 && ci[3] == 13);
  CHECK(rj[0] == 0 && rj[3] == 3);
  tables(4, 4, 0.0f, 10.0f, 1.0f, 20, 10.0, ci, rj);  // y in (-14, -10]: below the map
  for (int j = 0; j < 4; ++j) CHECK(rj[j] == -1);
  // straddling: x from -12 to 8 in steps of 1 against a costmap of [-5, 5) with 10 cells
  tables(3, 20, -12.0f, -1.5f, 1.0f, 10, 5.0, ci, rj);
  for (int i = 0; i < 20; ++i) {
    const double x = -12.0 + i + 0.5;
    CHECK(ci[i] == ((x >= -5.0 && x < 5.0) ? (int)std::floor(x + 5.0) : -1));
  }
  CHECK(ci[6] == -1 && ci[7] == 0 && ci[16] == 9 && ci[17] == -1);
  CHECK(rj[0] == 4 && rj[1] == 5 && rj[2] == 6);  // y centres 1, 0, -1 -> (5 - y) = 4, 5, 6
  // outside altogether, far enough for the index to leave int32 were it converted unchecked
  tables(5, 5, 1.0e12f, -3.0e12f, 1.0f, 16, 8.0, ci, rj);
  for (int k = 0; k < 5; ++k) CHECK(ci[k] == -1 && rj[k] == -1);
  tables(5, 5, -1.0e12f, 3.0e12f, 1.0f, 16, 8.0, ci, rj);
  for (int k = 0; k < 5; ++k) CHECK(ci[k] == -1 && rj[k] == -1);
  // non-commensurate: 160 cells against 33, every entry floor of the rule in float64
  const float res = (float)(150.0 / 160);
  tables(160, 160, -75.0f, -75.0f, res, 33, 75.0, ci, rj);
  const double rc = 150.0 / 33;
  for (int i = 0; i < 160; ++i) {
    CHECK(ci[i] == (int)std::floor((-75.0 + (i + 0.5) * (double)res + 75.0) / rc));
    CHECK(rj[i] == (int)std::floor((75.0 - (75.0 - (i + 0.5) * (double)res)) / rc));
  }
  // a costmap half-width smaller than the DEM's: the outer cells drop out on both sides
  tables(192, 192, -75.0f, -75.0f, 150.0f / 192, 24, 30.0, ci, rj);
  CHECK(ci[0] == -1 && ci[191] == -1 && rj[0] == -1 && rj[191] == -1 && ci[96] == 12 && rj[95] == 11);
}

static void check_threshold_and_cos() {
  int32_t T = -1;
  CHECK(hazard_threshold(7.0f, 24, 75.0, &T) && T == 1);   // (7 / 6.25)^2 = 1.25
  CHECK(hazard_threshold(7.0f, 33, 75.0, &T) && T == 2);   // (7 / 4.5454)^2 = 2.37
  CHECK(hazard_threshold(0.0f, 24, 75.0, &T) && T == 0);
  CHECK(hazard_threshold(6.25f, 24, 75.0, &T) && T == 1);  // exactly one cell
  CHECK(hazard_threshold(6.2f, 24, 75.0, &T) && T == 0);
  CHECK(hazard_threshold(1.3f, 750, 75.0, &T) && T == 42);  // 1.3f / 0.2 is a shade under 6.5, whose square is 42.25
  T = 77;
  CHECK(!hazard_threshold(3.0e5f, 8192, 10.0, &T) && T == 77);  // (1.2e8)^2 beyond int32: T untouched
  CHECK(hazard_threshold(46340.0f, 2, 1.0, &T) && T == 46340 * 46340);
  CHECK(!hazard_threshold(46341.0f, 2, 1.0, &T));  // 46341^2 = 2^31 + 4633
  CHECK(hazard_cos(60.0f) == (float)std::cos(60.0 * 3.141592653589793 / 180.0));
  CHECK(hazard_cos(10.0f) > hazard_cos(20.0f) && hazard_cos(89.0f) > 0.0f && hazard_cos(1.0f) < 1.0f);
}

static void check_refusals() {
  const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
  auto err = [](float deg, float infl, int32_t mc, int32_t rsv, int size = 24, double hw = 75.0) {
    mppi_hazard h{deg, infl, mc, rsv};
    return hazard_check(h, size, hw);
  };
  auto names = [](const std::string& e, const char* field) { return e.find(field) != std::string::npos; };
  CHECK(err(15.0f, 7.0f, 1, 0).empty());
  CHECK(err(15.0f, 0.0f, 64, 0).empty());
  CHECK(err(89.9f, 0.0f, 1, 0).empty() && err(0.001f, 0.0f, 1, 0).empty());
  for (float bad : {0.0f, -5.0f, 90.0f, 120.0f, inf, -inf, nan}) CHECK(names(err(bad, 1.0f, 1, 0), "max_slope_deg"));
  for (float bad : {-0.5f, inf, -inf, nan}) CHECK(names(err(15.0f, bad, 1, 0), "inflate"));
  CHECK(names(err(15.0f, 3.0e5f, 1, 0, 8192, 10.0), "inflate") && names(err(15.0f, 3.0e5f, 1, 0, 8192, 10.0), "int32"));
  CHECK(names(err(15.0f, 1.0f, 0, 0), "min_cells") && names(err(15.0f, 1.0f, -3, 0), "min_cells"));
  CHECK(names(err(15.0f, 1.0f, 1, 1), "reserved") && names(err(15.0f, 1.0f, 1, -1), "reserved"));
  CHECK(sizeof(mppi_hazard) == 16);
}

static void check_tiling() {
  // the window of a workgroup (kHzCols columns x R rows) fits the counters whenever lds is set
  struct Case {
    int rows, cols;
    double dem_hw;
    int size;
    double hw;
  };
  const Case cases[] = {{1500, 1500, 75.0, 750, 75.0}, {8192, 8192, 102.4, 1024, 102.4}, {192, 192, 75.0, 24, 75.0},
                        {1024, 1024, 50.0, 1024, 50.0}, {40, 40, 75.0, 128, 75.0},      {2, 2, 75.0, 24, 75.0},
                        {96, 130, 40.0, 33, 30.0},      {64, 64, 100.0, 8192, 100.0}};
  for (const Case& c : cases) {
    const float res = (float)(2 * c.dem_hw / c.cols);
    const HazardTiling t = hazard_tiling(c.rows, c.cols, res, c.size, c.hw);
    CHECK(t.rows_per_group >= kHzUnroll && t.rows_per_group <= kHzMaxRows && t.rows_per_group % kHzUnroll == 0);
    if (t.lds) {
      const double ratio = (double)res / (2 * c.hw / c.size);
      const double wi = std::ceil(std::min(c.cols, kHzCols) * ratio) + 1, wj = std::ceil(t.rows_per_group * ratio) + 1;
      CHECK(wi * wj <= kHzLdsCounters);
    }
  }
  CHECK(hazard_tiling(8192, 8192, 0.025f, 1024, 102.4).rows_per_group == 32);
  CHECK(hazard_tiling(8192, 8192, 0.025f, 1024, 102.4).lds);
  CHECK(hazard_tiling(1500, 1500, 0.1f, 750, 75.0).rows_per_group == 8);
  CHECK(!hazard_tiling(64, 64, 3.125f, 8192, 100.0).lds);  // 100 costmap cells per DEM cell: nothing to reduce
}

int main() {
  check_tables();
  check_threshold_and_cos();
  check_refusals();
  check_tiling();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("hazard tables ok\n");
  return 0;
}
