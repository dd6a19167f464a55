// C-ABI implementation (include/mppi.h): the on-device crater-field DEM builder (mppi_build_dem /
// mppi_dem_builder_* / mppi_batch_build_dem; Surface.create_surface, MPPI_isaac.py:307-356).
#include <hip/hip_runtime.h>

#include <memory>
#include <string>

#include "mppi.h"
#include "mppi_ctx.h"
#include "mppi_dem_build.h"
#include "mppi_dem_terms.h"

using namespace mppi;
using namespace mppi::capi;

namespace {

// Device scratch of one build: the crater rows, the two factor tables and the base.
struct DemScratch {
  DeviceBuf<double> craters, R, C;
  DeviceBuf<float> base;
};

int dem_variant_check(int32_t variant) {
  if (variant != MPPI_DEM_MFMA && variant != MPPI_DEM_VALU)
    return fail(MPPI_EINVAL, "DEM variant must be MPPI_DEM_MFMA or MPPI_DEM_VALU");
  return MPPI_OK;
}

int dem_args_check(const double* craters, int32_t n, int32_t grid, double half_width, int32_t variant) {
  const std::string why = dem_check(craters, n, grid, half_width);
  if (!why.empty()) return fail(MPPI_EINVAL, "DEM build: " + why);
  return dem_variant_check(variant);
}

// Uploads, the factor kernel and the product kernel on `st` (arguments already checked); the host
// arrays are pageable, so the caller waits for `st` before they go.  ev: null, or two events recorded
// around the two kernels.
int dem_enqueue(DemScratch& sc, hipStream_t st, const double* craters, int32_t n, int32_t grid, double half_width,
                const float* base_host, float* dst, int32_t variant, hipEvent_t* ev) {
  const int terms = (int)dem_terms_padded(n);
  const size_t cells = (size_t)grid * grid;
  if (n > 0) {
    int rc = grow(sc.craters, (size_t)n * 4 * sizeof(double), st);
    if (!rc) rc = grow(sc.R, (size_t)terms * grid * sizeof(double), st);
    if (!rc) rc = grow(sc.C, (size_t)terms * grid * sizeof(double), st);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(sc.craters, craters, (size_t)n * 4 * sizeof(double), hipMemcpyHostToDevice, st));
  }
  if (base_host) {
    if (int rc = grow(sc.base, cells * sizeof(float), st)) return rc;
    HIP_TRY(hipMemcpyAsync(sc.base, base_host, cells * sizeof(float), hipMemcpyHostToDevice, st));
  }
  if (ev) HIP_TRY(hipEventRecord(ev[0], st));
  HIP_TRY(launch_dem_factors(sc.craters, n, terms, grid, half_width, sc.R, sc.C, st));
  HIP_TRY(launch_dem_product(sc.R, sc.C, terms, grid, base_host ? sc.base.get() : nullptr, dst, variant, st));
  if (ev) HIP_TRY(hipEventRecord(ev[1], st));
  return MPPI_OK;
}

}  // namespace

int mppi::capi::build_dem_into(hipStream_t st, const double* craters, int32_t n, int32_t grid, double half_width,
                               const float* base_host, float* dst, float* out_host, int32_t variant) {
  if (int rc = dem_args_check(craters, n, grid, half_width, variant)) return rc;
  DemScratch sc;
  if (int rc = dem_enqueue(sc, st, craters, n, grid, half_width, base_host, dst, variant, nullptr)) return rc;
  if (out_host)
    HIP_TRY(hipMemcpyAsync(out_host, dst, (size_t)grid * grid * sizeof(float), hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  return MPPI_OK;
}

struct mppi_dem_builder {
  int device = 0;
  Stream stream;
  DemScratch sc;
  DeviceBuf<float> out;
  Event ev[2];
  double last_ms = 0;
};

namespace {

// The builder's launches between its two events, then the copy out and the wait.
template <class Enqueue>
int builder_run(mppi_dem_builder* b, int32_t grid, float* out_host, float* out_device, Enqueue enqueue) {
  HIP_TRY(hipSetDevice(b->device));
  const size_t bytes = (size_t)grid * grid * sizeof(float);
  if (!out_device)
    if (int rc = grow(b->out, bytes, b->stream)) return rc;
  float* dst = out_device ? out_device : b->out.get();
  hipEvent_t ev[2] = {b->ev[0], b->ev[1]};
  if (int rc = enqueue(dst, ev)) return rc;
  if (out_host) HIP_TRY(hipMemcpyAsync(out_host, dst, bytes, hipMemcpyDeviceToHost, b->stream));
  HIP_TRY(hipStreamSynchronize(b->stream));
  float ms = 0;
  HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
  b->last_ms = ms;
  return MPPI_OK;
}

}  // namespace

extern "C" {

int mppi_dem_builder_create(int32_t device, mppi_dem_builder** out) {
  if (!out) return fail(MPPI_EINVAL, "null argument");
  *out = nullptr;
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<mppi_dem_builder> b(new mppi_dem_builder());
  b->device = device;
  if (b->stream.create(hipStreamNonBlocking) || b->ev[0].create() || b->ev[1].create())
    return fail(MPPI_EHIP, "DEM builder: stream/event creation failed");
  *out = b.release();
  return MPPI_OK;
}

void mppi_dem_builder_destroy(mppi_dem_builder* b) {
  if (!b) return;
  hipSetDevice(b->device);
  if (b->stream) hipStreamSynchronize(b->stream);
  delete b;
}

int mppi_dem_builder_build(mppi_dem_builder* b, const double* craters, int32_t n, int32_t grid_size,
                           double half_width, const float* base_host, float* out_host, float* out_device,
                           int32_t variant) {
  if (!b) return fail(MPPI_EINVAL, "null builder");
  if (int rc = dem_args_check(craters, n, grid_size, half_width, variant)) return rc;
  return builder_run(b, grid_size, out_host, out_device, [&](float* dst, hipEvent_t* ev) {
    return dem_enqueue(b->sc, b->stream, craters, n, grid_size, half_width, base_host, dst, variant, ev);
  });
}

int mppi_dem_builder_product(mppi_dem_builder* b, const double* r_dev, const double* c_dev, int32_t terms,
                             int32_t grid_size, float* out_host, float* out_device, int32_t variant) {
  if (!b) return fail(MPPI_EINVAL, "null builder");
  if (terms < 0 || terms % kDemTermPad != 0) return fail(MPPI_EINVAL, "DEM product: terms must be a multiple of 4, >= 0");
  if (terms > 0 && (!r_dev || !c_dev)) return fail(MPPI_EINVAL, "DEM product: null factor table");
  if (grid_size < 2 || grid_size > kDemMaxGrid) return fail(MPPI_EINVAL, "DEM product: grid_size must be in [2, 32768]");
  if (int rc = dem_variant_check(variant)) return rc;
  return builder_run(b, grid_size, out_host, out_device, [&](float* dst, hipEvent_t* ev) {
    HIP_TRY(hipEventRecord(ev[0], b->stream));
    HIP_TRY(launch_dem_product(r_dev, c_dev, terms, grid_size, nullptr, dst, variant, b->stream));
    HIP_TRY(hipEventRecord(ev[1], b->stream));
    return (int)MPPI_OK;
  });
}

int mppi_dem_builder_last_ms(mppi_dem_builder* b, double* ms) {
  if (!b || !ms) return fail(MPPI_EINVAL, "null argument");
  *ms = b->last_ms;
  return MPPI_OK;
}

int mppi_build_dem(mppi_ctx* c, const double* craters, int32_t n, int32_t grid_size, double half_width,
                   const float* base_host, float* out_host, int32_t variant) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc = dem_args_check(craters, n, grid_size, half_width, variant)) return rc;
  const float res = (float)(2 * half_width / grid_size);  // Surface.resolution (MPPI_isaac.py:265)
  return install_dem(c, grid_size, grid_size, -(float)half_width, -(float)half_width, res, [&](float* dst) {
    return build_dem_into(c->stream, craters, n, grid_size, half_width, base_host, dst, out_host, variant);
  });
}

int mppi_batch_build_dem(mppi_batch* b, int32_t slot, const double* craters, int32_t n, double half_width,
                         const float* base_host, float* out_host, int32_t variant) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  mppi_ctx* c = batch_context(b);
  // (the slot index, then the context's DEM, then the arguments: as mppi_batch_set_dem orders its refusals)
  if (int rc = batch_dem_slot(b, slot)) return rc;
  if (!c->dem.Z || c->dem.rows <= 0)
    return fail(MPPI_ESTATE, "batch_build_dem: no DEM: call mppi_set_dem first (a slot takes the context's geometry)");
  const int grid = c->dem.rows;
  if (c->dem.cols != grid) return fail(MPPI_EINVAL, "batch_build_dem: the context's DEM is not square");
  if (!(half_width > 0) || c->dem.x_min != -(float)half_width || c->dem.y_min != -(float)half_width)
    return fail(MPPI_EINVAL, "batch_build_dem: the context's DEM is not centred (x_min = y_min = -half_width)");
  if (c->dem.res != (float)(2 * half_width / grid))
    return fail(MPPI_EINVAL, "batch_build_dem: the context DEM's resolution is not 2 * half_width / rows");
  if (int rc = dem_args_check(craters, n, grid, half_width, variant)) return rc;
  return batch_fill_dem(b, slot, "batch_build_dem", [&](float* dst) {
    return build_dem_into(c->stream, craters, n, grid, half_width, base_host, dst, out_host, variant);
  });
}

}  // extern "C"
