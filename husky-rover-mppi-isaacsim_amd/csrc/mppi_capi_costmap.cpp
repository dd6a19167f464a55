// C-ABI implementation (include/mppi.h): the obstacle costmap builder (mppi_build_costmap / mppi_costmap_builder_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <memory>
#include <string>
#include <vector>

#include "mppi.h"
#include "mppi_ctx.h"
#include "mppi_costmap.h"
#include "mppi_hazard.h"

using namespace mppi;
using namespace mppi::capi;

namespace {

int costmap_check(const double* obstacles, int32_t n, int32_t size, int32_t power, int32_t metric) {
  if (n < 0 || (n > 0 && !obstacles)) return fail(MPPI_EINVAL, "obstacles: null pointer or negative count");
  if (metric != MPPI_COSTMAP_CHAMFER5 && metric != MPPI_COSTMAP_EXACT && metric != MPPI_COSTMAP_CHAMFER5_RASTER)
    return fail(MPPI_EINVAL, "costmap metric must be MPPI_COSTMAP_CHAMFER5, MPPI_COSTMAP_EXACT or MPPI_COSTMAP_CHAMFER5_RASTER");
  if (size < 2 || size > COSTMAP_MAX_SIZE) return fail(MPPI_EINVAL, "costmap size must be in [2, 8192]");
  if (power < 0) return fail(MPPI_EINVAL, "costmap power must be >= 0");
  return MPPI_OK;
}

// Host staging for one build, with float64 arithmetic in the reference's order
// (MPPI_isaac.py:363-370): x_local = y_global - y0, y_local = x_global - x0,
// total_radius = r_obs/2 + r_robot + 0.1, squared with libm pow as CPython's `**`;
// grid coordinates as np.linspace(-hw, hw, size) (i*step + start, last = stop).
// The vectors must outlive the stream work (the caller synchronises).
int costmap_stage(CostmapBuffers& sc, const double* obstacles, int32_t n, int32_t size, double hw, double ox,
                  double oy, double r_robot, std::vector<double>& obs, std::vector<double>& xs, hipStream_t st) {
  const size_t cells = (size_t)size * size;
  const size_t nseg = (size_t)(size + COSTMAP_SEG - 1) / COSTMAP_SEG;
  if (cells > sc.cells_cap) {
    HIP_TRY(hipStreamSynchronize(st));
    sc.drop_planes();
    HIP_TRY(sc.occ.alloc(cells));
    HIP_TRY(sc.first.alloc(nseg * size * sizeof(int32_t)));
    HIP_TRY(sc.last.alloc(nseg * size * sizeof(int32_t)));
    HIP_TRY(sc.g2.alloc(cells * sizeof(int32_t)));
    HIP_TRY(sc.d2.alloc(cells * sizeof(int32_t)));
    HIP_TRY(sc.lines.alloc(16 * cells * sizeof(uint32_t)));
    sc.cells_cap = cells;
  }
  if (!sc.range) HIP_TRY(sc.range.alloc((2 + 2 * COSTMAP_MAX_SIZE) * sizeof(int32_t)));
  const size_t nobs = (size_t)std::max<int32_t>(n, 1);
  int rc = grow(sc.obs, nobs * 3 * sizeof(double), st);
  if (!rc) rc = grow(sc.xs, (size_t)size * sizeof(double), st);
  if (rc) return rc;
  obs.assign(nobs * 3, 0.0);
  for (int32_t k = 0; k < n; ++k) {
    const double xg = obstacles[3 * k], yg = obstacles[3 * k + 1], r = obstacles[3 * k + 2];
    const double tr = r / 2 + r_robot + 0.1;
    obs[3 * k + 0] = yg - oy;
    obs[3 * k + 1] = xg - ox;
    obs[3 * k + 2] = std::pow(tr, 2.0);
  }
  xs.resize(size);
  const double start = -hw, stop = hw;
  const double step = (stop - start) / (double)(size - 1);
  for (int32_t i = 0; i < size; ++i) xs[i] = (double)i * step + start;
  xs[size - 1] = stop;
  HIP_TRY(hipMemcpyAsync(sc.obs, obs.data(), nobs * 3 * sizeof(double), hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemcpyAsync(sc.xs, xs.data(), (size_t)size * sizeof(double), hipMemcpyHostToDevice, st));
  return MPPI_OK;
}

// The hazard part of a build: the refusals, the two tables to the device, the
// mask plane, and the kernels' argument block.  `tab` must outlive the stream work.
int hazard_stage(CostmapBuffers& sc, const mppi_hazard& hz, const DemView& d, int32_t size, double hw, bool want_mask,
                 hipStream_t st, std::vector<int32_t>& tab, CostmapHazard& out) {
  const std::string err = hazard_check(hz, size, hw);
  if (!err.empty()) return fail(MPPI_EINVAL, err);
  std::vector<int32_t> ci, rj;
  hazard_tables(d.rows, d.cols, d.x_min, d.y_min, d.res, size, hw, ci, rj);
  tab = ci;
  tab.insert(tab.end(), rj.begin(), rj.end());
  int rc = grow(sc.hz_tab, tab.size() * sizeof(int32_t), st);
  if (!rc && want_mask) rc = grow(sc.mask, (size_t)size * size, st);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(sc.hz_tab, tab.data(), tab.size() * sizeof(int32_t), hipMemcpyHostToDevice, st));
  out.Z = d.Z;
  out.rows = d.rows;
  out.cols = d.cols;
  out.res = d.res;
  out.cos_limit = hazard_cos(hz.max_slope_deg);
  out.ci = sc.hz_tab;
  out.rj = sc.hz_tab + d.cols;
  out.min_cells = hz.min_cells;
  hazard_threshold(hz.inflate, size, hw, &out.T);
  const HazardTiling t = hazard_tiling(d.rows, d.cols, d.res, size, hw);
  out.rows_per_group = t.rows_per_group;
  out.lds = t.lds;
  out.mask = want_mask ? sc.mask.get() : nullptr;
  return MPPI_OK;
}

}  // namespace

// The build on the context's stream and scratch into `dst` (device, size x size floats), copied to
// out_host when given; ends synchronised.  mppi_build_costmap and a batch's costmap slots
// (mppi_batch_build_costmap) share it.
int mppi::capi::build_costmap_into(mppi_ctx* c, const double* obstacles, int32_t n, int32_t size, double half_width,
                                   double origin_x, double origin_y, double r_robot, int32_t power, int32_t metric,
                                   float* dst, float* out_host, const mppi_hazard* hz, const DemView* dem,
                                   uint8_t* mask_host) {
  int rc = costmap_check(obstacles, n, size, power, metric);
  if (rc) return rc;
  std::vector<double> obs, xs;
  std::vector<int32_t> tab;
  CostmapHazard ha;
  rc = costmap_stage(c->cmap.scratch, obstacles, n, size, half_width, origin_x, origin_y, r_robot, obs, xs, c->stream);
  if (!rc && hz) rc = hazard_stage(c->cmap.scratch, *hz, *dem, size, half_width, mask_host != nullptr, c->stream, tab, ha);
  if (rc) return rc;
  HIP_TRY(launch_costmap_build(c->cmap.scratch.view(), n, size, power, dst, c->stream, metric, hz ? &ha : nullptr));
  if (out_host)
    HIP_TRY(hipMemcpyAsync(out_host, dst, (size_t)size * size * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (hz && mask_host)
    HIP_TRY(hipMemcpyAsync(mask_host, ha.mask, (size_t)size * size, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

struct mppi_costmap_builder {
  int device = 0;
  Stream stream;
  CostmapBuffers sc;
  DeviceBuf<float> out;
  Event ev[2];
  Event ev_count[2];  // around the hazard count kernel
  double last_ms = 0;
  double count_ms = 0;  // the count kernel of the last hazard build (0: none)
};

extern "C" {

int mppi_build_costmap(mppi_ctx* c, const double* obstacles, int32_t n, int32_t size, double half_width,
                       double origin_x, double origin_y, double r_robot, int32_t power, float* out_host,
                       int32_t metric) {
  return mppi_build_costmap_hazard(c, obstacles, n, size, half_width, origin_x, origin_y, r_robot, power, nullptr,
                                   out_host, nullptr, metric);
}

int mppi_build_costmap_hazard(mppi_ctx* c, const double* obstacles, int32_t n, int32_t size, double half_width,
                              double origin_x, double origin_y, double r_robot, int32_t power, const mppi_hazard* hz,
                              float* out_host, uint8_t* mask_host, int32_t metric) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = costmap_check(obstacles, n, size, power, metric);
  if (rc) return rc;
  DemView dem;
  if (hz) {
    const std::string err = hazard_check(*hz, size, half_width);
    if (!err.empty()) return fail(MPPI_EINVAL, err);
    if (!c->dem.Z || c->dem.rows <= 0)
      return fail(MPPI_ESTATE, "build_costmap_hazard: no DEM bound: call mppi_set_dem first");
    dem = dem_view(c->dem);
  }
  const float res = (float)(2 * half_width / size);  // Surface.costmap_resolution (MPPI_isaac.py:272)
  if (!(res > 0.0f)) return fail(MPPI_EINVAL, "costmap resolution must be > 0");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)size * size * sizeof(float);
  rc = grow(c->cmap.cm, bytes, c->stream);
  if (rc) return rc;
  rc = build_costmap_into(c, obstacles, n, size, half_width, origin_x, origin_y, r_robot, power, metric, c->cmap.cm,
                          out_host, hz, &dem, mask_host);
  if (rc) return rc;
  c->cmap.size = size;
  c->cmap.hw = (float)half_width;
  c->cmap.res = res;
  return verified_reciprocal(c, res, &c->cmap.rinv_res);
}

int mppi_costmap_builder_create(int32_t device, mppi_costmap_builder** out) {
  if (!out) return fail(MPPI_EINVAL, "null argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<mppi_costmap_builder> b(new mppi_costmap_builder());
  b->device = device;
  if (b->stream.create(hipStreamNonBlocking) || b->ev[0].create() || b->ev[1].create())
    return fail(MPPI_EHIP, "costmap builder: stream/event creation failed");
  if (b->ev_count[0].create() || b->ev_count[1].create())
    return fail(MPPI_EHIP, "costmap builder: stream/event creation failed");
  *out = b.release();
  return MPPI_OK;
}

void mppi_costmap_builder_destroy(mppi_costmap_builder* b) {
  if (!b) return;
  hipSetDevice(b->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  delete b;
}

int mppi_costmap_builder_build(mppi_costmap_builder* b, const double* obstacles, int32_t n, int32_t size,
                               double half_width, double origin_x, double origin_y, double r_robot, int32_t power,
                               float* out_host, float* out_device, int32_t metric) {
  return mppi_costmap_builder_build_hazard(b, obstacles, n, size, half_width, origin_x, origin_y, r_robot, power,
                                           nullptr, 0, 0, 0.0f, 0.0f, 0.0f, nullptr, out_host, out_device, nullptr,
                                           metric);
}

int mppi_costmap_builder_build_hazard(mppi_costmap_builder* b, const double* obstacles, int32_t n, int32_t size,
                                      double half_width, double origin_x, double origin_y, double r_robot,
                                      int32_t power, const float* z_device, int32_t rows, int32_t cols, float x_min,
                                      float y_min, float resolution, const mppi_hazard* hz, float* out_host,
                                      float* out_device, uint8_t* mask_host, int32_t metric) {
  if (!b) return fail(MPPI_EINVAL, "null builder");
  int rc = costmap_check(obstacles, n, size, power, metric);
  if (rc) return rc;
  if (hz) {
    const std::string err = hazard_check(*hz, size, half_width);
    if (!err.empty()) return fail(MPPI_EINVAL, err);
    if (!z_device) return fail(MPPI_ESTATE, "costmap_builder_build_hazard: no DEM: z_device is null");
    if (rows < 2 || cols < 2 || rows > 32768 || cols > 32768)
      return fail(MPPI_EINVAL, "costmap_builder_build_hazard: rows and cols must be in [2, 32768]");
    if (!std::isfinite(resolution) || !(resolution > 0.0f) || !std::isfinite(x_min) || !std::isfinite(y_min))
      return fail(MPPI_EINVAL, "costmap_builder_build_hazard: x_min, y_min must be finite and resolution finite and > 0");
  }
  HIP_TRY(hipSetDevice(b->device));
  const size_t bytes = (size_t)size * size * sizeof(float);
  if (!out_device) {
    rc = grow(b->out, bytes, b->stream);
    if (rc) return rc;
  }
  float* dst = out_device ? out_device : b->out;
  std::vector<double> obs, xs;
  rc = costmap_stage(b->sc, obstacles, n, size, half_width, origin_x, origin_y, r_robot, obs, xs, b->stream);
  std::vector<int32_t> tab;
  CostmapHazard ha;
  if (!rc && hz)
    rc = hazard_stage(b->sc, *hz, DemView{z_device, rows, cols, x_min, y_min, resolution}, size, half_width,
                      mask_host != nullptr, b->stream, tab, ha);
  if (rc) return rc;
  ha.ev_count[0] = b->ev_count[0];
  ha.ev_count[1] = b->ev_count[1];
  HIP_TRY(hipEventRecord(b->ev[0], b->stream));
  HIP_TRY(launch_costmap_build(b->sc.view(), n, size, power, dst, b->stream, metric, hz ? &ha : nullptr));
  HIP_TRY(hipEventRecord(b->ev[1], b->stream));
  if (out_host) HIP_TRY(hipMemcpyAsync(out_host, dst, bytes, hipMemcpyDeviceToHost, b->stream));
  if (hz && mask_host) HIP_TRY(hipMemcpyAsync(mask_host, ha.mask, (size_t)size * size, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  b->last_ms = ms;
  b->count_ms = 0;
  if (hz) {
    HIP_TRY(hipEventElapsedTime(&ms, b->ev_count[0], b->ev_count[1]));
    b->count_ms = ms;
  }
  return MPPI_OK;
}

int mppi_costmap_builder_hazard_count_ms(mppi_costmap_builder* b, double* ms) {
  if (!b || !ms) return fail(MPPI_EINVAL, "null argument");
  *ms = b->count_ms;
  return MPPI_OK;
}

int mppi_costmap_builder_last_ms(mppi_costmap_builder* b, double* ms) {
  if (!b || !ms) return fail(MPPI_EINVAL, "null argument");
  *ms = b->last_ms;
  return MPPI_OK;
}

}  // extern "C"
