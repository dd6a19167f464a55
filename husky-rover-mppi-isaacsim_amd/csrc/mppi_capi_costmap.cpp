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

}  // namespace

// The build on the context's stream and scratch into `dst` (device, size x size floats), copied to
// out_host when given; ends synchronised.  mppi_build_costmap and a batch's costmap slots
// (mppi_batch_build_costmap) share it.
int mppi::capi::build_costmap_into(mppi_ctx* c, const double* obstacles, int32_t n, int32_t size, double half_width,
                                   double origin_x, double origin_y, double r_robot, int32_t power, int32_t metric,
                                   float* dst, float* out_host) {
  int rc = costmap_check(obstacles, n, size, power, metric);
  if (rc) return rc;
  std::vector<double> obs, xs;
  rc = costmap_stage(c->cmap.scratch, obstacles, n, size, half_width, origin_x, origin_y, r_robot, obs, xs, c->stream);
  if (rc) return rc;
  HIP_TRY(launch_costmap_build(c->cmap.scratch.view(), n, size, power, dst, c->stream, metric));
  if (out_host)
    HIP_TRY(hipMemcpyAsync(out_host, dst, (size_t)size * size * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

struct mppi_costmap_builder {
  int device = 0;
  Stream stream;
  CostmapBuffers sc;
  DeviceBuf<float> out;
  Event ev[2];
  double last_ms = 0;
};

extern "C" {

int mppi_build_costmap(mppi_ctx* c, const double* obstacles, int32_t n, int32_t size, double half_width,
                       double origin_x, double origin_y, double r_robot, int32_t power, float* out_host,
                       int32_t metric) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = costmap_check(obstacles, n, size, power, metric);
  if (rc) return rc;
  const float res = (float)(2 * half_width / size);  // Surface.costmap_resolution (MPPI_isaac.py:272)
  if (!(res > 0.0f)) return fail(MPPI_EINVAL, "costmap resolution must be > 0");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)size * size * sizeof(float);
  rc = grow(c->cmap.cm, bytes, c->stream);
  if (rc) return rc;
  rc = build_costmap_into(c, obstacles, n, size, half_width, origin_x, origin_y, r_robot, power, metric, c->cmap.cm,
                          out_host);
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
  if (!b) return fail(MPPI_EINVAL, "null builder");
  int rc = costmap_check(obstacles, n, size, power, metric);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(b->device));
  const size_t bytes = (size_t)size * size * sizeof(float);
  if (!out_device) {
    rc = grow(b->out, bytes, b->stream);
    if (rc) return rc;
  }
  float* dst = out_device ? out_device : b->out;
  std::vector<double> obs, xs;
  rc = costmap_stage(b->sc, obstacles, n, size, half_width, origin_x, origin_y, r_robot, obs, xs, b->stream);
  if (rc) return rc;
  HIP_TRY(hipEventRecord(b->ev[0], b->stream));
  HIP_TRY(launch_costmap_build(b->sc.view(), n, size, power, dst, b->stream, metric));
  HIP_TRY(hipEventRecord(b->ev[1], b->stream));
  if (out_host) HIP_TRY(hipMemcpyAsync(out_host, dst, bytes, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  b->last_ms = ms;
  return MPPI_OK;
}

int mppi_costmap_builder_last_ms(mppi_costmap_builder* b, double* ms) {
  if (!b || !ms) return fail(MPPI_EINVAL, "null argument");
  *ms = b->last_ms;
  return MPPI_OK;
}

}  // extern "C"
