// Host check of the crater-field DEM builder's bookkeeping (csrc/mppi_dem_terms.h): packing of n craters
// into 2n terms, the padding, the LDS chunk counts and the argument checks.  Built with ASan + UBSan by
// tests/test_dem_terms.py; the header needs no HIP header.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <string>
#include <vector>

#include "mppi_dem_terms.h"

using namespace mppi;

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static std::vector<double> craters(int n) {
  std::vector<double> c((size_t)n * 4);
  for (int k = 0; k < n; ++k) {
    c[4 * k + 0] = -3.0 + 0.01 * k;
    c[4 * k + 1] = 2.0 - 0.02 * k;
    c[4 * k + 2] = 0.6 + 0.003 * k;
    c[4 * k + 3] = 0.5 + 0.002 * k;
  }
  return c;
}

static void check_packing() {
  const int ns[5] = {0, 1, 2, 3, 1100};
  const int padded[5] = {0, 4, 4, 8, 2200};
  for (int i = 0; i < 5; ++i) {
    const int n = ns[i];
    CHECK(dem_terms(n) == 2 * n);
    CHECK(dem_terms_padded(n) == padded[i]);
    CHECK(dem_terms_padded(n) % kDemTermPad == 0 && dem_terms_padded(n) >= 2 * n && dem_terms_padded(n) < 2 * n + kDemTermPad);
    const std::vector<double> c = craters(n);
    const std::vector<double> t = dem_pack_terms(c.data(), n);  // (exactly sized: ASan sees an overrun)
    CHECK((int64_t)t.size() == 4 * dem_terms_padded(n));
    for (int k = 0; k < n; ++k) {
      const double h = c[4 * k + 2], w = c[4 * k + 3];
      const double* rim = &t[(size_t)(2 * k) * 4];
      const double* bowl = rim + 4;
      CHECK(rim[0] == h - 0.5 && rim[1] == 2.0 * (w * w));
      CHECK(bowl[0] == -(h + 0.5) && bowl[1] == 2.0 * ((w / 2.0) * (w / 2.0)));
      CHECK(rim[2] == c[4 * k] && rim[3] == c[4 * k + 1] && bowl[2] == c[4 * k] && bowl[3] == c[4 * k + 1]);
    }
    for (int64_t p = 2 * n; p < dem_terms_padded(n); ++p)  // padding: zero amplitude, a harmless divisor
      CHECK(t[(size_t)p * 4] == 0.0 && t[(size_t)p * 4 + 1] == 1.0);
  }
}

static void check_chunks() {
  CHECK(kDemChunk == 32 && kDemChunk % kDemTermPad == 0);
  CHECK(2 * kDemChunk * kDemTile * (int)sizeof(double) <= kDemLdsBudget);
  CHECK(dem_chunk_terms(kDemLdsBudget) == 32);
  CHECK(dem_chunk_terms(kDemLdsBudget - 1) == 28);   // one byte short of 32 terms: the multiple of 4 below
  CHECK(dem_chunk_terms(64 * 1024) == 64);
  CHECK(dem_chunk_terms(4 * 1024) == 4);
  CHECK(dem_chunk_terms(4 * 1024 - 1) == 0);         // not even one group of 4 terms
  CHECK(dem_chunk_count(0) == 0);
  CHECK(dem_chunk_count(4) == 1);
  CHECK(dem_chunk_count(32) == 1);
  CHECK(dem_chunk_count(36) == 2);
  CHECK(dem_chunk_count(64) == 2);
  CHECK(dem_chunk_count(2200) == 69);                // 68 full chunks and one of 24 terms
  CHECK(dem_chunk_count(2200, 64) == 35);
}

static void check_linspace() {
  const double hw = 6.5;
  const int grid = 130;
  const double step = dem_linspace_step(hw, grid);
  CHECK(step == 13.0 / 129.0);
  CHECK(dem_coord(0, grid, hw, step) == -hw);
  CHECK(dem_coord(grid - 1, grid, hw, step) == hw);
  CHECK(dem_coord(7, grid, hw, step) == 7.0 * step + (-hw));
}

static bool names(const std::string& msg, const char* a, const char* b) {
  return msg.find(a) != std::string::npos && msg.find(b) != std::string::npos;
}

static void check_refusals() {
  const double inf = std::numeric_limits<double>::infinity(), nan = std::nan("");
  std::vector<double> c = craters(3);
  CHECK(dem_check(c.data(), 3, 130, 6.5).empty());
  CHECK(dem_check(nullptr, 0, 2, 1.0).empty());
  CHECK(names(dem_check(c.data(), -1, 130, 6.5), "n", ">= 0"));
  CHECK(names(dem_check(nullptr, 2, 130, 6.5), "craters", "null"));
  CHECK(names(dem_check(c.data(), 3, 1, 6.5), "grid_size", ">= 2"));
  CHECK(names(dem_check(c.data(), 3, kDemMaxGrid + 1, 6.5), "grid_size", "<="));
  CHECK(names(dem_check(c.data(), 3, 130, 0.0), "half_width", "> 0"));
  CHECK(names(dem_check(c.data(), 3, 130, -1.0), "half_width", "> 0"));
  CHECK(names(dem_check(c.data(), 3, 130, inf), "half_width", "finite"));
  CHECK(names(dem_check(c.data(), 3, 130, nan), "half_width", "finite"));
  static const char* const field[4] = {"cx", "cy", "height", "width"};
  for (int k = 0; k < 3; ++k)
    for (int f = 0; f < 4; ++f)
      for (double bad : {inf, -inf, nan}) {
        std::vector<double> d = c;
        d[4 * k + f] = bad;
        const std::string who = "crater " + std::to_string(k) + ":";
        CHECK(names(dem_check(d.data(), 3, 130, 6.5), who.c_str(), field[f]));
      }
  std::vector<double> d = c;
  d[4 * 2 + 3] = 0.0;
  CHECK(names(dem_check(d.data(), 3, 130, 6.5), "crater 2:", "width"));
  d[4 * 2 + 3] = -0.0;
  CHECK(names(dem_check(d.data(), 3, 130, 6.5), "crater 2:", "width"));
  d[4 * 2 + 3] = 1e-170;  // non-zero, but its square is 0: the divisor would be
  CHECK(names(dem_check(d.data(), 3, 130, 6.5), "crater 2:", "width"));
  d[4 * 2 + 3] = 1e160;   // its square overflows
  CHECK(names(dem_check(d.data(), 3, 130, 6.5), "crater 2:", "width"));
  d[4 * 2 + 3] = -1.5;    // a negative width is the reference's too: it is squared
  CHECK(dem_check(d.data(), 3, 130, 6.5).empty());
}

int main() {
  check_packing();
  check_chunks();
  check_linspace();
  check_refusals();
  if (g_fail) {
    std::printf("%d check(s) failed\n", g_fail);
    return 1;
  }
  std::printf("dem terms ok\n");
  return 0;
}
