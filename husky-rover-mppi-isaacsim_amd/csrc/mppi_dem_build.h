// On-device crater-field DEM builder (mppi_dem_build.hip): launch functions.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace mppi {

// The two factor tables of `terms` (padded, a multiple of kDemTermPad) terms, term-major
// [terms][grid] float64: R[t][i] = a_t exp(-((y_i - cy_t)^2) / s_t), C[t][j] = exp(-((x_j - cx_t)^2) / s_t),
// from the n crater rows (cx, cy, height, width) in device memory.
hipError_t launch_dem_factors(const double* craters, int n, int terms, int grid, double half_width, double* R,
                              double* C, hipStream_t st);
// out[i][j] = float32( sum_t R[t][i] C[t][j] + base[i][j] ) (base may be null), float64 accumulation,
// one rounding.  variant: MPPI_DEM_MFMA / MPPI_DEM_VALU.  terms = 0: the base, or zeros.
hipError_t launch_dem_product(const double* R, const double* C, int terms, int grid, const float* base, float* out,
                              int variant, hipStream_t st);

}  // namespace mppi
