// C-ABI implementation (include/mppi.h): path scoring and per-critic cost terms (mppi_score.hip).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>
#include <vector>

#include "mppi.h"
#include "mppi_ctx.h"
#include "mppi_score.h"

using namespace mppi;
using namespace mppi::capi;

namespace mppi {
namespace capi {

// One launch of the scoring kernel on the context stream, bracketed by HIP events (score_ms).  Waits
// for the stream.
int run_score(mppi_ctx* c, const ScoreArgs& a) {
  Event ev[2];
  hipError_t e = (hipError_t)ev[0].create();
  if (e == hipSuccess) e = (hipError_t)ev[1].create();
  if (e == hipSuccess) e = hipEventRecord(ev[0], c->stream);
  if (e == hipSuccess) e = launch_score(a, c->stream);
  if (e == hipSuccess) e = hipEventRecord(ev[1], c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  float ms = 0.0f;
  if (e == hipSuccess) e = hipEventElapsedTime(&ms, ev[0], ev[1]);
  if (e != hipSuccess) return fail(MPPI_EHIP, std::string("score: ") + hipGetErrorString(e));
  c->tm.score_ms = ms;
  return MPPI_OK;
}

}  // namespace capi
}  // namespace mppi

namespace {

// Score n device-resident paths of `stride` waypoints from `st` (x, y, goal) with the context's
// costmap and critic parameters; the kernel is bracketed by HIP events (score_ms).  Waits for the stream.
int score_device(mppi_ctx* c, int64_t n, int32_t stride, const int32_t* lengths, const float* traj,
                 const float* lw, const float* rw, const float* v, const mppi_state& st, float* cost,
                 float* terms, int32_t* collisions, float* orient = nullptr) {
  const mppi_params& p = c->p;
  ServerCmd d;
  state_fields(p, st, d);
  ScoreArgs a;
  std::memset(&a, 0, sizeof(a));
  a.traj = traj;
  // the critic set's slope mode: the body form is the kernel without wheel arrays
  const bool body = c->crit.slope_mode == MPPI_SLOPE_BODY;
  a.lw = body ? nullptr : lw;
  a.rw = body ? nullptr : rw;
  a.w_orient = c->crit.w_orientation;
  a.x0 = d.x0;
  a.y0 = d.y0;
  a.orient = orient;
  a.v = v;
  a.lengths = lengths;
  a.n = n;
  a.stride = stride;
  a.cm = c->cmap.cm;
  a.cm_size = c->cmap.size;
  a.hw = c->cmap.hw;
  a.res_c = c->cmap.res;
  a.gx = d.gx;
  a.gy = d.gy;
  a.igx = d.igx;
  a.igy = d.igy;
  a.pf_scale = d.pf_scale;
  a.pf_far = d.pf_far;
  a.speed_on = d.speed_on;
  a.vmax = p.v_max_linear;
  a.thr = p.collision_threshold;
  a.pen = p.collision_penalty;
  a.w_path = p.w_path;
  a.w_slope = p.w_slope;
  a.w_speed = p.w_speed;
  a.w_obs = p.w_obstacle;
  a.cost = cost;
  a.terms = terms;
  a.collisions = collisions;
  return run_score(c, a);
}

}  // namespace

extern "C" {

int mppi_score_paths(mppi_ctx* c, int64_t n, int32_t stride, const int32_t* lengths, const float* traj,
                     const float* left_wheel, const float* right_wheel, const float* lin_vel,
                     const mppi_state* origin, mppi_path_scores* out) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  if (!traj || !lin_vel || !out) return fail(MPPI_EINVAL, "score_paths: null traj, lin_vel or out");
  if (n < 0 || stride < 1) return fail(MPPI_EINVAL, "score_paths: need n >= 0 and stride >= 1");
  if ((left_wheel == nullptr) != (right_wheel == nullptr))
    return fail(MPPI_EINVAL, "score_paths: give both wheel arrays or neither");
  if (n * (int64_t)stride >= ((int64_t)1 << 31)) return fail(MPPI_EINVAL, "score_paths: n * stride must be below 2^31");
  if (lengths)
    for (int64_t i = 0; i < n; ++i)
      if (lengths[i] < 1 || lengths[i] > stride)
        return fail(MPPI_EINVAL, "score_paths: lengths[" + std::to_string(i) + "] outside [1, stride]");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "score_paths: no costmap: call mppi_set_costmap first");
  if (!origin && !c->sb.have_state) return fail(MPPI_ESTATE, "score_paths: no origin and no state set");
  if (n == 0) return MPPI_OK;
  const mppi_state st = origin ? *origin : c->sb.st;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const bool wheels = left_wheel != nullptr;
  const size_t nS = (size_t)n * stride;
  // one allocation, every array 16-byte aligned: [traj][lw][rw][v][lengths][cost][terms][collisions]
  const size_t b3 = up16(3 * nS * sizeof(float)), b1 = up16(nS * sizeof(float)), bn = up16((size_t)n * 4);
  const size_t bytes = b3 * (wheels ? 3 : 1) + b1 + bn * 3 + up16((size_t)n * 16);
  DeviceBuf<char> buf;
  HIP_TRY(buf.alloc(bytes));
  char* q = buf;
  float* d_traj = (float*)q;
  q += b3;
  float* d_lw = nullptr;
  float* d_rw = nullptr;
  if (wheels) {
    d_lw = (float*)q;
    q += b3;
    d_rw = (float*)q;
    q += b3;
  }
  float* d_v = (float*)q;
  q += b1;
  int32_t* d_len = (int32_t*)q;
  q += bn;
  float* d_cost = (float*)q;
  q += bn;
  float* d_terms = (float*)q;
  q += up16((size_t)n * 16);
  int32_t* d_col = (int32_t*)q;
  hipError_t e = hipMemcpyAsync(d_traj, traj, 3 * nS * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && wheels) e = hipMemcpyAsync(d_lw, left_wheel, 3 * nS * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && wheels) e = hipMemcpyAsync(d_rw, right_wheel, 3 * nS * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d_v, lin_vel, nS * sizeof(float), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && lengths) e = hipMemcpyAsync(d_len, lengths, (size_t)n * 4, hipMemcpyHostToDevice, c->stream);
  int rc = MPPI_OK;
  if (e == hipSuccess)
    rc = score_device(c, n, stride, lengths ? d_len : nullptr, d_traj, d_lw, d_rw, d_v, st, d_cost, d_terms, d_col);
  if (e == hipSuccess && rc == MPPI_OK && out->cost) e = hipMemcpyAsync(out->cost, d_cost, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == MPPI_OK && out->terms) e = hipMemcpyAsync(out->terms, d_terms, (size_t)n * 16, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == MPPI_OK && out->collisions) e = hipMemcpyAsync(out->collisions, d_col, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == MPPI_OK) e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  if (e != hipSuccess) return fail(MPPI_EHIP, std::string("score_paths: ") + hipGetErrorString(e));
  return MPPI_OK;
}

}  // extern "C"

namespace {

// mppi_get_cost_terms (orient == false: terms [K*4]) and mppi_get_cost_terms5 (terms [K*5])
int cost_terms(mppi_ctx* c, float* terms, int32_t* collisions, bool orient) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->last.have) return fail(MPPI_ESTATE, "no step to score");
  const int64_t K = c->p.num_trajectories;
  const int H = H_of(c);
  const size_t KH = (size_t)K * H;
  if (KH == 0) return MPPI_OK;
  if (KH >= ((size_t)1 << 31)) return fail(MPPI_EINVAL, "cost_terms: K * H must be below 2^31");
  // device-side dump buffers for traj, lw, rw, v only, and the 20 bytes per trajectory that leave
  DeviceBuf<float> dev[4];
  const size_t cnt[4] = {3 * KH, 3 * KH, 3 * KH, KH};
  DeviceBuf<float> d_terms, d_po;
  DeviceBuf<int32_t> d_col;
  std::vector<float> t4, po;
  int out_rc = MPPI_OK;
  if (orient) {
    if (d_po.alloc((size_t)K * 4)) out_rc = fail(MPPI_EHIP, "cost_terms allocation failed");
    t4.resize((size_t)K * 4);
    po.resize((size_t)K);
  }
  for (int i = 0; i < 4 && out_rc == MPPI_OK; ++i)
    if (dev[i].alloc(cnt[i] * sizeof(float))) out_rc = fail(MPPI_EHIP, "cost_terms allocation failed");
  if (out_rc == MPPI_OK && (d_terms.alloc((size_t)K * 16) || d_col.alloc((size_t)K * 4)))
    out_rc = fail(MPPI_EHIP, "cost_terms allocation failed");
  if (out_rc == MPPI_OK) {
    RolloutArgs d;
    std::memset(&d, 0, sizeof(d));
    d.d_traj = dev[0];
    d.d_lw = dev[1];
    d.d_rw = dev[2];
    d.d_v = dev[3];
    // re-run the last step (deterministic: costs/records are rewritten with identical values)
    out_rc = enqueue_rollout(c, c->last.proj, c->last.step, c->last.mode, c->last.plan,
                             c->sb.u_nom[c->last.nominal], c->last.state, &d);
    if (out_rc == MPPI_OK)
      out_rc = score_device(c, K, H, nullptr, dev[0], dev[1], dev[2], dev[3], c->last.state, nullptr, d_terms, d_col,
                            orient ? d_po.get() : nullptr);
    if (out_rc == MPPI_OK && terms &&
        hipMemcpyAsync(orient ? t4.data() : terms, d_terms, (size_t)K * 16, hipMemcpyDeviceToHost, c->stream) !=
            hipSuccess)
      out_rc = fail(MPPI_EHIP, "cost_terms copy failed");
    if (out_rc == MPPI_OK && terms && orient &&
        hipMemcpyAsync(po.data(), d_po, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
      out_rc = fail(MPPI_EHIP, "cost_terms copy failed");
    if (out_rc == MPPI_OK && collisions &&
        hipMemcpyAsync(collisions, d_col, (size_t)K * 4, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
      out_rc = fail(MPPI_EHIP, "cost_terms copy failed");
    if (out_rc == MPPI_OK && hipStreamSynchronize(c->stream) != hipSuccess) out_rc = fail(MPPI_EHIP, "cost_terms sync failed");
    if (out_rc == MPPI_OK && terms && orient)
      for (int64_t k = 0; k < K; ++k) {
        std::memcpy(terms + 5 * k, t4.data() + 4 * k, 16);
        terms[5 * k + 4] = po[(size_t)k];
      }
  }
  return out_rc;
}

}  // namespace

extern "C" {

int mppi_get_cost_terms(mppi_ctx* c, float* terms, int32_t* collisions) {
  return cost_terms(c, terms, collisions, false);
}

int mppi_get_cost_terms5(mppi_ctx* c, float* terms5, int32_t* collisions) {
  return cost_terms(c, terms5, collisions, true);
}

int mppi_get_score_ms(mppi_ctx* c, double* ms) {
  if (!c || !ms) return fail(MPPI_EINVAL, "null argument");
  *ms = c->tm.score_ms;
  return MPPI_OK;
}

int mppi_detmath_atan2(mppi_ctx* c, int64_t n, const double* y, const double* x, double* dm, double* dev) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (n < 0 || n > ((int64_t)1 << 28)) return fail(MPPI_EINVAL, "detmath_atan2: n must be in [0, 2^28]");
  if (n == 0) return MPPI_OK;
  if (!y || !x || !dm || !dev) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)n * sizeof(double);
  DeviceBuf<double> buf;
  HIP_TRY(buf.alloc(4 * bytes));
  double* d = buf;
  hipError_t e = hipMemcpyAsync(d, y, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d + n, x, bytes, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_atan2_probe(d, d + n, n, d + 2 * n, d + 3 * n, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dm, d + 2 * n, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(dev, d + 3 * n, bytes, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(MPPI_EHIP, std::string("detmath_atan2: ") + hipGetErrorString(e));
  return MPPI_OK;
}

}  // extern "C"
