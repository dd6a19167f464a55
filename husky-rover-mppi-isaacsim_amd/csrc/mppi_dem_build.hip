// Crater-field DEMs on the GPU (Surface.create_surface, MPPI_isaac.py:307-356), as the separable sum
// Z = R^T C of DESIGN.md §3.6 / §4: every gaussian of the reference splits into a row factor and a
// column factor, so a field of n craters is one [grid x 2n] . [2n x grid] float64 product.
//   dem_factor_kernel   the two factor tables from the crater rows
//   dem_product_kernel  the product on v_mfma_f64_16x16x4_f64, plus the base, rounded once to float32
//   dem_product_valu_kernel  the same product on the vector ALU (the A/B, and the tests' second opinion)
// No workgroup waits for another, no atomics; every global access is bounds-checked against `grid`.
#include <hip/hip_runtime.h>

#include "mppi.h"
#include "mppi_dem_build.h"
#include "mppi_dem_terms.h"

namespace mppi {

namespace {

constexpr int kDemThreads = 256;

__global__ __launch_bounds__(kDemThreads) void dem_factor_kernel(const double* __restrict__ craters, int n, int terms,
                                                                 int grid, double hw, double step,
                                                                 double* __restrict__ R, double* __restrict__ C) {
  const size_t idx = (size_t)blockIdx.x * kDemThreads + threadIdx.x;
  if (idx >= (size_t)terms * grid) return;
  const int t = (int)(idx / grid), i = (int)(idx % grid);
  double p[4];  // a, s, cx, cy
  dem_packed_term(craters, n, t, p);
  if (t >= 2 * n) {  // padding: a zero-amplitude term
    R[idx] = 0.0;
    C[idx] = 0.0;
    return;
  }
  const double x = dem_coord(i, grid, hw, step);  // y_i = x_i
  const double dy = x - p[3], dx = x - p[2];
  R[idx] = p[0] * exp(-(dy * dy) / p[1]);
  C[idx] = exp(-(dx * dx) / p[1]);
}

// Chunk [t0, t0 + kc) of both tables for the tile at (r0, c0) into LDS; cells past the grid read as 0.
__device__ __forceinline__ void dem_stage(const double* __restrict__ R, const double* __restrict__ C, int t0, int kc,
                                          int grid, int r0, int c0, double (*sR)[kDemTile], double (*sC)[kDemTile]) {
  for (int e = threadIdx.x; e < kc * kDemTile; e += kDemThreads) {
    const int k = e / kDemTile, x = e % kDemTile;
    const size_t row = (size_t)(t0 + k) * grid;
    sR[k][x] = r0 + x < grid ? R[row + r0 + x] : 0.0;
    sC[k][x] = c0 + x < grid ? C[row + c0 + x] : 0.0;
  }
}

__device__ __forceinline__ void dem_store(double z, int row, int col, int grid, const float* __restrict__ base,
                                          float* __restrict__ out) {
  if (row >= grid || col >= grid) return;
  const size_t o = (size_t)row * grid + col;
  if (base) z += (double)base[o];
  out[o] = (float)z;
}

typedef double dem_acc4 __attribute__((ext_vector_type(4)));

// 64 x 64 outputs per workgroup, four waves as 2 x 2, each a 32 x 32 block of 2 x 2 MFMA tiles.
// v_mfma_f64_16x16x4_f64: lane l gives A[row l & 15][k = l >> 4] and B[k = l >> 4][col l & 15]; result
// register r of lane l is D[row (l >> 4) + 4 r][col l & 15] (not the f32 map).
__global__ __launch_bounds__(kDemThreads) void dem_product_kernel(const double* __restrict__ R,
                                                                  const double* __restrict__ C, int terms, int grid,
                                                                  const float* __restrict__ base,
                                                                  float* __restrict__ out) {
  __shared__ double sR[kDemChunk][kDemTile];
  __shared__ double sC[kDemChunk][kDemTile];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int r0 = blockIdx.y * kDemTile, c0 = blockIdx.x * kDemTile;
  const int wr = (wave >> 1) * 32, wc = (wave & 1) * 32;
  const int lk = lane >> 4, lx = lane & 15;
  dem_acc4 acc[2][2] = {};
  for (int t0 = 0; t0 < terms; t0 += kDemChunk) {
    const int kc = min(kDemChunk, terms - t0);  // a multiple of kDemTermPad, the same for every thread
    dem_stage(R, C, t0, kc, grid, r0, c0, sR, sC);
    __syncthreads();
    for (int k = 0; k < kc; k += kDemTermPad) {
      const double a0 = sR[k + lk][wr + lx], a1 = sR[k + lk][wr + 16 + lx];
      const double b0 = sC[k + lk][wc + lx], b1 = sC[k + lk][wc + 16 + lx];
      acc[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, acc[0][0], 0, 0, 0);
      acc[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, acc[0][1], 0, 0, 0);
      acc[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, acc[1][0], 0, 0, 0);
      acc[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, acc[1][1], 0, 0, 0);
    }
    __syncthreads();
  }
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int q = 0; q < 2; ++q)
#pragma unroll
      for (int r = 0; r < 4; ++r)
        dem_store(acc[m][q][r], r0 + wr + 16 * m + lk + 4 * r, c0 + wc + 16 * q + lx, grid, base, out);
}

// The same tile on the vector ALU: thread (ty, tx) of 16 x 16 holds rows ty + 16 r, columns tx + 16 c.
__global__ __launch_bounds__(kDemThreads) void dem_product_valu_kernel(const double* __restrict__ R,
                                                                       const double* __restrict__ C, int terms,
                                                                       int grid, const float* __restrict__ base,
                                                                       float* __restrict__ out) {
  __shared__ double sR[kDemChunk][kDemTile];
  __shared__ double sC[kDemChunk][kDemTile];
  const int ty = threadIdx.x >> 4, tx = threadIdx.x & 15;
  const int r0 = blockIdx.y * kDemTile, c0 = blockIdx.x * kDemTile;
  double acc[4][4] = {};
  for (int t0 = 0; t0 < terms; t0 += kDemChunk) {
    const int kc = min(kDemChunk, terms - t0);
    dem_stage(R, C, t0, kc, grid, r0, c0, sR, sC);
    __syncthreads();
    for (int k = 0; k < kc; ++k) {
      double a[4], b[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) a[r] = sR[k][ty + 16 * r];
#pragma unroll
      for (int c = 0; c < 4; ++c) b[c] = sC[k][tx + 16 * c];
#pragma unroll
      for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = __builtin_fma(a[r], b[c], acc[r][c]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int r = 0; r < 4; ++r)
#pragma unroll
    for (int c = 0; c < 4; ++c) dem_store(acc[r][c], r0 + ty + 16 * r, c0 + tx + 16 * c, grid, base, out);
}

}  // namespace

hipError_t launch_dem_factors(const double* craters, int n, int terms, int grid, double half_width, double* R,
                              double* C, hipStream_t st) {
  if (terms <= 0) return hipSuccess;
  const size_t cells = (size_t)terms * grid;
  const size_t blocks = (cells + kDemThreads - 1) / kDemThreads;
  if (blocks > 0x7fffffffu) return hipErrorInvalidValue;
  hipLaunchKernelGGL(dem_factor_kernel, dim3((unsigned)blocks), dim3(kDemThreads), 0, st, craters, n, terms, grid,
                     half_width, dem_linspace_step(half_width, grid), R, C);
  return hipGetLastError();
}

hipError_t launch_dem_product(const double* R, const double* C, int terms, int grid, const float* base, float* out,
                              int variant, hipStream_t st) {
  if (terms % kDemTermPad != 0 || grid < 1) return hipErrorInvalidValue;
  const unsigned tiles = (unsigned)((grid + kDemTile - 1) / kDemTile);
  if (variant == MPPI_DEM_VALU)
    hipLaunchKernelGGL(dem_product_valu_kernel, dim3(tiles, tiles), dim3(kDemThreads), 0, st, R, C, terms, grid, base,
                       out);
  else
    hipLaunchKernelGGL(dem_product_kernel, dim3(tiles, tiles), dim3(kDemThreads), 0, st, R, C, terms, grid, base,
                       out);
  return hipGetLastError();
}

}  // namespace mppi
