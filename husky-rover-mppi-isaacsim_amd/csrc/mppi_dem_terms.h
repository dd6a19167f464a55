// The bookkeeping of the on-device crater-field DEM builder (mppi_build_dem / mppi_dem_builder_* /
// mppi_batch_build_dem), as plain arithmetic (no HIP header, so
// tests/native/dem_terms_check.cpp checks it on the host): how n craters of
// Surface.create_surface (MPPI_isaac.py:307-320) become 2n separable terms, how the term count is
// padded for the product kernel, how many LDS chunks the factor tables are staged in, and the
// argument checks.  dem_term is the one statement of the term formula: the factor kernel
// (mppi_dem_build.hip) calls it on the device, the host check on the host.
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#ifdef __HIPCC__
#define MPPI_DEM_HD __host__ __device__
#else
#define MPPI_DEM_HD
#endif

namespace mppi {

constexpr int kDemTermPad = 4;    // terms one v_mfma_f64_16x16x4_f64 consumes: the term count is padded to it
constexpr int kDemTile = 64;      // output rows and columns per workgroup
constexpr int kDemLdsBudget = 32 * 1024;  // bytes of LDS for the two staged factor chunks
constexpr int kDemMaxGrid = 32768;        // the builder's own limit (a context's DEM has check_grid's)

// Terms (padded) of n craters: two per crater, then zero-amplitude terms up to a multiple of kDemTermPad.
constexpr int64_t dem_terms(int64_t n) { return 2 * n; }
constexpr int64_t dem_terms_padded(int64_t n) { return (2 * n + kDemTermPad - 1) / kDemTermPad * kDemTermPad; }

// Terms per LDS chunk for a budget: two tables of [chunk][tile] doubles, a multiple of kDemTermPad (0
// when not even one group of kDemTermPad terms fits).
constexpr int dem_chunk_terms(int lds_bytes, int tile = kDemTile) {
  return lds_bytes / (2 * tile * (int)sizeof(double)) / kDemTermPad * kDemTermPad;
}
constexpr int kDemChunk = dem_chunk_terms(kDemLdsBudget);
static_assert(kDemChunk == 32, "32 terms x 64 cells x 8 bytes x 2 tables = 32 KiB");
// Chunks the product kernel's term loop takes for `terms` (padded) terms.
constexpr int64_t dem_chunk_count(int64_t terms, int chunk = kDemChunk) { return (terms + chunk - 1) / chunk; }

// One term (amplitude a, divisor s) of a crater row (cx, cy, height, width), float64 as the reference
// computes them (MPPI_isaac.py:319-320): which = 0 the rim gaussian (height - 0.5, 2 width^2), which = 1
// the bowl (-(height + 0.5), 2 (width/2)^2).
MPPI_DEM_HD inline void dem_term(const double* crater, int which, double* a, double* s) {
  const double h = crater[2], w = crater[3];
  if (which == 0) {
    *a = h - 0.5;
    *s = 2.0 * (w * w);
  } else {
    const double w2 = w / 2.0;
    *a = -(h + 0.5);
    *s = 2.0 * (w2 * w2);
  }
}

// Term t of the padded list as (a, s, cx, cy); t >= 2n is a zero-amplitude padding term (s = 1).
MPPI_DEM_HD inline void dem_packed_term(const double* craters, int64_t n, int64_t t, double* out4) {
  if (t >= 2 * n) {
    out4[0] = 0.0;
    out4[1] = 1.0;
    out4[2] = 0.0;
    out4[3] = 0.0;
    return;
  }
  const double* c = craters + 4 * (t >> 1);
  dem_term(c, (int)(t & 1), &out4[0], &out4[1]);
  out4[2] = c[0];
  out4[3] = c[1];
}

// The padded term list [dem_terms_padded(n)][4] on the host (the restatement the kernel is checked against).
inline std::vector<double> dem_pack_terms(const double* craters, int64_t n) {
  const int64_t T = dem_terms_padded(n);
  std::vector<double> out((size_t)T * 4);
  for (int64_t t = 0; t < T; ++t) dem_packed_term(craters, n, t, &out[(size_t)t * 4]);
  return out;
}

// np.linspace(-hw, hw, grid)[j] (float64): j * step + start, one multiply and one add, the last point
// hw itself.  (Not fused: the library is built with -ffp-contract=off.)
MPPI_DEM_HD inline double dem_linspace_step(double hw, int grid) { return (hw - (-hw)) / (double)(grid - 1); }
MPPI_DEM_HD inline double dem_coord(int j, int grid, double hw, double step) {
  return j == grid - 1 ? hw : (double)j * step + (-hw);
}

// The argument checks of every build.  Empty string: fine; else the refusal, naming the crater and the field.
inline std::string dem_check(const double* craters, int64_t n, int64_t grid, double half_width) {
  if (n < 0) return "craters: n must be >= 0";
  if (n > 0 && !craters) return "craters: null pointer";
  if (n > (int64_t)1 << 28) return "craters: n above 2^28";
  if (grid < 2) return "grid_size must be >= 2";
  if (grid > kDemMaxGrid) return "grid_size must be <= " + std::to_string(kDemMaxGrid);
  if (!std::isfinite(half_width) || !(half_width > 0.0)) return "half_width must be finite and > 0";
  static const char* const field[4] = {"cx", "cy", "height", "width"};
  for (int64_t k = 0; k < n; ++k) {
    const double* c = craters + 4 * k;
    for (int f = 0; f < 4; ++f)
      if (!std::isfinite(c[f])) return "crater " + std::to_string(k) + ": " + field[f] + " must be finite";
    if (c[3] == 0.0) return "crater " + std::to_string(k) + ": width must be non-zero";
    double a, s;
    dem_term(c, 1, &a, &s);
    const double s0 = 2.0 * (c[3] * c[3]);
    if (!(s > 0.0) || !std::isfinite(s0))
      return "crater " + std::to_string(k) + ": width: 2 width^2 and 2 (width/2)^2 must be finite and non-zero";
  }
  return std::string();
}

}  // namespace mppi
