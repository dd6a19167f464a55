// C-ABI implementation (include/mppi.h): bilinear DEM lookup and query binning.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <string>

#include "mppi.h"
#include "mppi_ctx.h"

using namespace mppi;
using namespace mppi::capi;

extern "C" {

int mppi_bilinear_query(mppi_ctx* c, const float* x, const float* y, float* h, int64_t n) {
  if (!c || !x || !y || !h) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM");
  if (n < 0) return fail(MPPI_EINVAL, "n < 0");
  HIP_TRY(hipSetDevice(c->device));
  if (n == 0) return MPPI_OK;
  HIP_TRY(launch_bilinear(c->dem.Z, c->dem.rows, c->dem.cols, c->dem.x_min, c->dem.y_min, c->dem.res, x, y, h, n, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_bilinear_tiles(mppi_ctx* c, int32_t* ntiles) {
  if (!c || !ntiles) return fail(MPPI_EINVAL, "null argument");
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM");
  *ntiles = ((c->dem.rows + BIL_TILE - 1) / BIL_TILE) * ((c->dem.cols + BIL_TILE - 1) / BIL_TILE);
  return MPPI_OK;
}

int mppi_bin_queries(mppi_ctx* c, const float* x, const float* y, int64_t n, float* xs_out, float* ys_out,
                     int32_t* perm, int32_t* tile_off) {
  if (!c || !x || !y || !xs_out || !ys_out || !perm || !tile_off) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM");
  if (n < 0 || n > INT32_MAX) return fail(MPPI_EINVAL, "n out of range [0, 2^31)");
  HIP_TRY(hipSetDevice(c->device));
  int32_t nt = 0;
  mppi_bilinear_tiles(c, &nt);
  // the histogram and scatter kernels keep one counter per tile in LDS: a skinny DEM (one side
  // under 128 cells) can have more tiles than that holds
  if ((size_t)nt * sizeof(int) > kLdsBytes - 1024)
    return fail(MPPI_EINVAL, "bin_queries: " + std::to_string(nt) + " tiles of 128 x 128 cells exceed the LDS "
                             "histogram (at most " + std::to_string((kLdsBytes - 1024) / sizeof(int)) +
                             "); use mppi_bilinear_query for this DEM");
  const size_t hist = (size_t)bin_chunks(n, nt) * nt;  // [chunks][tiles] per-chunk histograms
  BinScratch& bin = c->bin;
  int rc = grow(bin.tile_of, std::max<size_t>(hist, 1) * sizeof(int), c->stream);
  // counts [nt], then the tile-row cursors of the two-level scatter [nt] (rows of tiles <= nt)
  if (!rc) rc = grow(bin.counts, 2 * (size_t)nt * sizeof(int), c->stream);
  if (!rc) rc = grow(bin.cursor, (size_t)nt * sizeof(int), c->stream);
  if (!rc) rc = grow(bin.cx, (size_t)n * sizeof(float), c->stream);
  if (!rc) rc = grow(bin.cy, (size_t)n * sizeof(float), c->stream);
  if (!rc) rc = grow(bin.ci, (size_t)n * sizeof(int32_t), c->stream);
  if (rc) return rc;
  const Dem& dem = c->dem;
  HIP_TRY(launch_bin_queries(x, y, n, dem.x_min, dem.y_min, dem.res, dem.rinv_res, dem.rinv_res != 0.0f, dem.rows,
                             dem.cols, bin.tile_of, bin.counts, bin.cursor, tile_off, xs_out, ys_out, perm,
                             c->stream, bin.cx, bin.cy, bin.ci, bin.counts + nt));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_bilinear_tiled(mppi_ctx* c, const float* xs, const float* ys, const int32_t* tile_off, float* h) {
  if (!c || !xs || !ys || !tile_off || !h) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_bilinear_tiled(c->dem.Z, c->dem.rows, c->dem.cols, c->dem.x_min, c->dem.y_min, c->dem.res, c->dem.rinv_res,
                                c->dem.rinv_res != 0.0f, xs, ys, h, tile_off, c->stream));
  return MPPI_OK;
}

}  // extern "C"
