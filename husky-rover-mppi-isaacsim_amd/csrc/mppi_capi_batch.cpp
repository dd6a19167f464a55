// C-ABI implementation (include/mppi.h): batched closed-loop episodes (mppi_batch_*).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "mppi.h"
#include "mppi_batch_scene.h"
#include "mppi_batch_tasks.h"
#include "mppi_batch_wheels.h"
#include "mppi_ctx.h"
#include "mppi_path_metrics.h"
#include "mppi_score.h"

using namespace mppi;
using namespace mppi::capi;

struct mppi_batch {
  mppi_ctx* c = nullptr;
  int E = 0, blocks = 0, H = 0;
  std::vector<BatchEpisode> host;     // the table as last read from / written to the device
  std::vector<unsigned char> is_set;  // mppi_batch_set_episode was called for the episode
  DeviceBuf<BatchEpisode> ep;
  DeviceBuf<float> eps;
  DeviceBuf<float> unom;
  DeviceBuf<double> nodes;
  DeviceBuf<float> cost;
  DeviceBuf<float> fin;
  DeviceBuf<float> log;
  int log_cap = 0;
  PinnedBuf<int> active_count;
  Event ev[2];
  double last_ms = 0;
  bool failed = false;  // a HIP error of the batch: further runs are refused
  // mppi_batch_step_device: is_set in device memory (the ingest kernel's `active` rule), and whether
  // steps were enqueued that no synchronous call has waited for yet (a HIP error of theirs surfaces
  // in that call, which then refuses the batch as a failed run does)
  DeviceBuf<int> d_set;
  bool unwaited = false;
  // per-episode parameter variants (mppi_batch_set_variants / _set_episode_variant)
  std::vector<mppi_batch_variant> variants;  // the table as last set
  std::vector<int> ep_var;                   // [E] each episode's row, -1: none
  DeviceBuf<BatchVariant> d_var;             // [kBatchMaxVariants]
  DeviceBuf<int> d_ep_var;                   // [E]
  // the variant rows' critic sets (mppi_batch_set_variant_critics): row i belongs to variant row i
  std::vector<mppi_critics> critics;         // as last set
  DeviceBuf<BatchCriticRow> d_crit;          // [kBatchMaxVariants], rows past the set: slope_mode -1
  // the variant rows' sampling plans (mppi_batch_set_variant_sampling): row i belongs to variant row i
  std::vector<mppi_sampling> sampling;       // as last set
  DeviceBuf<SamplePlan> d_samp;              // [kBatchMaxVariants], rows past the set: antithetic -1
  // [E] x, y, goal_x, goal_y of each episode when its most recent run began (mppi_batch_score)
  std::vector<std::array<float, 4>> origin;
  // per-episode scenes and trajectory counts (mppi_batch_set_dem / _set_costmap / _set_episode_scene /
  // _set_episode_trajectories): `book` decides, the rest is the slots' memory and the kernels' tables
  BatchSceneBook book;
  std::vector<Dem> dems;              // [kBatchMaxDems] a live slot owns its heights and normal table
  std::vector<DeviceBuf<float>> cms;  // [kBatchMaxCostmaps]
  DeviceBuf<BatchSceneTable> d_tab;   // the slots' pointer tables and the [E] records (BatchArgs::scene)
  // the task queue (mppi_batch_set_tasks / _run_tasks): `tbook` decides, the rest is the list as given,
  // the device's tables and the host's copy of the results
  BatchTaskBook tbook;
  std::vector<mppi_batch_task> tasks;
  std::vector<BatchTaskResult> res;  // [N] as last read; a running task's is its lane's state
  DeviceBuf<BatchTask> d_tasks;
  DeviceBuf<BatchTaskResult> d_res;
  DeviceBuf<BatchLane> d_lane;       // [E]
  DeviceBuf<int> d_count;            // [1 + E] the next unclaimed task, then each lane's steps of the campaign
  DeviceBuf<float> tlog;             // the log arena, [sum of max_steps][8]
  std::vector<int> lane_steps;       // [E] as last read
  enum Campaign { kNotStarted, kUnfinished, kComplete } campaign = kNotStarted;
  // a scored list (mppi_batch_set_tasks_scored): the yardstick as taken when the list was set (each run
  // takes the costmap as it stands then), the lanes' accumulator records and the tasks' score rows
  bool scored = false;
  BatchYardstick yard{};
  DeviceBuf<BatchScoreAcc> d_acc;     // [E]
  DeviceBuf<BatchTaskScore> d_score;  // [N]
  // tracked device steps (mppi_batch_set_tracking): the yardstick and the caps as taken when tracking
  // was set (the pointers and the scene are filled in by each step), the episodes' tracking records,
  // their run counts and the results table
  bool tracking = false;
  BatchTrack trk{};
  float trk_goal_tol = 0.0f;           // the goal test's tolerance (the untracked step reads no policy)
  DeviceBuf<BatchTrackRec> d_track;    // [E]
  DeviceBuf<int> d_runs;               // [E]
  DeviceBuf<BatchRunResult> d_runres;  // [E][runs_per_episode]
  // wheel contacts and path metrics of executed paths (mppi_batch_set_wheel_log / _set_score_options): the
  // options as last set, read by the next run, list or tracking; then what each of those took, and the
  // tables, which exist only while their option is on
  BatchWheelBook wbook;                   // decides (mppi_batch_wheels.h); the rest is the tables it names
  DeviceBuf<float> wlog;                  // [E][log_cap][6], parallel to log: exists iff wbook.log_wheels()
  DeviceBuf<float> twlog;                 // the arena's parallel array, [rows of the arena][6]
  DeviceBuf<BatchWheelAcc> d_wacc;        // [E] a scored list's lanes
  DeviceBuf<PathMetricsAcc> d_macc;       // [E]
  DeviceBuf<PathMetrics> d_metrics;       // [N] beside d_score
  DeviceBuf<BatchWheelAcc> d_twacc;       // [E] tracked runs
  DeviceBuf<PathMetricsAcc> d_tmacc;      // [E]
  DeviceBuf<PathMetrics> d_runmetrics;    // [E][runs_per_episode] beside d_runres
};
static_assert(sizeof(mppi_path_metrics) == sizeof(PathMetrics), "mppi_path_metrics layout");
static_assert(kWheelSlopeWheels == MPPI_SLOPE_WHEELS && kWheelSlopeBody == MPPI_SLOPE_BODY, "mppi_slope_mode");
static_assert(sizeof(mppi_batch_variant) == sizeof(BatchVariant), "mppi_batch_variant layout");
static_assert(sizeof(mppi_critics) == sizeof(BatchCriticRow), "mppi_critics layout");
static_assert(sizeof(SceneRecord) == sizeof(BatchScene), "SceneRecord is BatchScene field for field");

namespace {

BatchVariant device_variant(const mppi_batch_variant& v) {
  BatchVariant r;
  r.w_path = v.w_path;
  r.w_slope = v.w_slope;
  r.w_speed = v.w_speed;
  r.w_obs = v.w_obstacle;
  r.thr = v.collision_threshold;
  r.pen = v.collision_penalty;
  r.T = v.temperature;
  r.fk = v.filter_k;
  r.fa = v.filter_a;
  r.ok = v.opt_filter_k;
  r.oa = v.opt_filter_a;
  r.sigma_base = v.sigma_base;
  r.sigma_div = v.sigma_div;
  r.proj = v.proj;
  return r;
}

int batch_episode(mppi_batch* b, int32_t e) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (e < 0 || e >= b->E) return fail(MPPI_EINVAL, "episode index out of range");
  return MPPI_OK;
}

SceneGeom dem_geom(const mppi_ctx* c) {
  return SceneGeom{c->dem.rows, c->dem.cols, c->dem.x_min, c->dem.y_min, c->dem.res};
}
SceneGeom costmap_geom(const mppi_ctx* c) { return SceneGeom{c->cmap.size, 0, c->cmap.hw, c->cmap.res, 0.0f}; }

// Episode e's scene record host -> device (synchronous), unless it still equals `before`.
int push_scene(mppi_batch* b, int e, const SceneRecord& before) {
  const SceneRecord r = b->book.record(e);
  if (std::memcmp(&r, &before, sizeof(r)) == 0) return MPPI_OK;
  HIP_TRY(hipMemcpyAsync(b->d_tab->rec + e, &r, sizeof(r), hipMemcpyHostToDevice, b->c->stream));
  HIP_TRY(hipStreamSynchronize(b->c->stream));
  return MPPI_OK;
}

// Every slot an episode in use holds still has the context's geometry (the launch's rinv_res, cdiv
// and plan are the context's): not after a mppi_set_dem / mppi_set_costmap of another size in between.
int scene_geometry(const mppi_batch* b) {
  int s = b->book.mismatch(kSceneDem, dem_geom(b->c));
  if (s >= 0)
    return fail(MPPI_ESTATE, "batch: DEM slot " + std::to_string(s) +
                                 " was set with another geometry than the context's current DEM");
  s = b->book.mismatch(kSceneCostmap, costmap_geom(b->c));
  if (s >= 0)
    return fail(MPPI_ESTATE, "batch: costmap slot " + std::to_string(s) +
                                 " was set with another geometry than the context's current costmap");
  return MPPI_OK;
}

int slot_index(const mppi_batch* b, SceneKind k, int32_t slot) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (!b->book.in_range(k, slot))
    return fail(MPPI_EINVAL, std::string(k == kSceneDem ? "DEM" : "costmap") + " slot " + std::to_string(slot) +
                                 " outside [0, " + std::to_string(b->book.slots(k)) + ")");
  return MPPI_OK;
}

// Free the slot unless an episode or a task of the list holds it.  (Its entry of the device table goes stale: no record names it.)
int slot_free(mppi_batch* b, SceneKind k, int32_t slot) {
  int who = b->tbook.holder(k, slot);
  if (who >= 0)
    return fail(MPPI_EINVAL, std::string(k == kSceneDem ? "DEM" : "costmap") + " slot " + std::to_string(slot) +
                                 " is held by task " + std::to_string(who) + " of the task list");
  if (b->book.free_slot(k, slot, &who) == kSceneSlotHeld)
    return fail(MPPI_EINVAL, std::string(k == kSceneDem ? "DEM" : "costmap") + " slot " + std::to_string(slot) +
                                 " is held by episode " + std::to_string(who));
  if (k == kSceneDem)
    b->dems[slot] = Dem{};
  else
    b->cms[slot].reset();
  return MPPI_OK;
}

// A buffer of `bytes` for a slot: `cur` when it is large enough, else a new one in `fresh` (`cur`
// stays as it is until the caller moves `fresh` in).  A failure leaves the batch usable.
template <class T>
int slot_alloc(const DeviceBuf<T>& cur, DeviceBuf<T>& fresh, size_t bytes, const char* what, int32_t slot) {
  if (cur && bytes <= cur.cap()) return MPPI_OK;
  if (fresh.alloc(bytes)) {
    (void)hipGetLastError();
    return fail(MPPI_EHIP, std::string(what) + " slot " + std::to_string(slot) + ": allocation of " +
                               std::to_string(bytes) + " bytes failed");
  }
  return MPPI_OK;
}

// The costmap slot's buffer for the context costmap's size (`fresh` holds a new one until the caller
// has filled it), or the error.
int costmap_slot_buffer(mppi_batch* b, int32_t slot, const char* who, DeviceBuf<float>& fresh, float** dst) {
  mppi_ctx* c = b->c;
  if (!c->cmap.cm || c->cmap.size <= 0)
    return fail(MPPI_ESTATE, std::string(who) + ": no costmap: call mppi_set_costmap first (a slot takes the context's geometry)");
  const size_t bytes = (size_t)c->cmap.size * c->cmap.size * sizeof(float);
  if (int rc = slot_alloc(b->cms[slot], fresh, bytes, "costmap", slot)) return rc;
  *dst = fresh ? fresh.get() : b->cms[slot].get();
  return MPPI_OK;
}

// The filled buffer becomes the slot's contents (synchronous).
int costmap_slot_publish(mppi_batch* b, int32_t slot, DeviceBuf<float>& fresh) {
  mppi_ctx* c = b->c;
  if (fresh) b->cms[slot] = std::move(fresh);
  const float* p = b->cms[slot];
  HIP_TRY(hipMemcpyAsync(b->d_tab->cms + slot, &p, sizeof(p), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  b->book.set_slot(kSceneCostmap, slot, costmap_geom(c));
  return MPPI_OK;
}

// The episode table device -> host (waits for the context stream).
int batch_pull(mppi_batch* b) {
  mppi_ctx* c = b->c;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(b->host.data(), b->ep, (size_t)b->E * sizeof(BatchEpisode), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

// The launches' scene and parameters; the kernels patch the episode's part.
void step_args(mppi_ctx* c, const Plan& pl, RolloutArgs& a, FinishArgs& f) {
  const mppi_state none{};
  fill_rollout(c, pl, none, 0, nullptr, a);
  a.clk = nullptr;
  a.rec_m = nullptr;
  a.ustore = nullptr;
  a.inj_u1 = a.inj_u2 = nullptr;
  a.k_offset = c->p.k_offset;
  fill_finish(c, pl, none, f);
  f.mode = 2;
}

// The noise launch's plans: the context's as it is now, and the rows' table while rows are set.
BatchNoisePlan noise_plan(const mppi_batch* b) {
  BatchNoisePlan np;
  np.ctx = device_plan(b->c->samp);
  np.rows = b->sampling.empty() ? nullptr : b->d_samp.get();
  return np;
}

// The batch's own part of the kernels' arguments: no variant table, no scene table and no log yet.
BatchArgs batch_args(mppi_batch* b, int proj, const mppi_loop_policy& pol) {
  const mppi_ctx* c = b->c;
  BatchArgs z{};
  z.ep_var = b->d_ep_var;
  z.proj = proj;
  z.ep = b->ep;
  z.E = b->E;
  z.blocks = b->blocks;
  z.H = b->H;
  z.k_pad = (int64_t)b->blocks * 256;
  z.eps = b->eps;
  z.unom = b->unom;
  z.nodes = b->nodes;
  z.cost = b->cost;
  z.fin = b->fin;
  z.sigma_base = pol.sigma_base;
  z.sigma_div = pol.sigma_div;
  z.goal_tol = pol.goal_tol;
  z.horizon = c->p.horizon;
  z.rwheel = c->p.robot_radius;
  z.active_count = b->active_count;
  z.crit = b->critics.empty() ? nullptr : b->d_crit.get();  // (read behind a variant index only)
  return z;
}

// The scorer's yardstick: the caller's row where one is given, else the context's parameters; the
// geometry of the context's costmap and its orientation weight as they stand now.
BatchYardstick resolve_yardstick(const mppi_ctx* c, const mppi_batch_variant* yardstick) {
  const mppi_params& p = c->p;
  BatchYardstick y{};
  y.hw = c->cmap.hw;
  y.res_c = c->cmap.res;
  y.vmax = p.v_max_linear;
  y.thr = yardstick ? yardstick->collision_threshold : p.collision_threshold;
  y.pen = yardstick ? yardstick->collision_penalty : p.collision_penalty;
  y.w_path = yardstick ? yardstick->w_path : p.w_path;
  y.w_slope = yardstick ? yardstick->w_slope : p.w_slope;
  y.w_speed = yardstick ? yardstick->w_speed : p.w_speed;
  y.w_obs = yardstick ? yardstick->w_obstacle : p.w_obstacle;
  y.w_orient = c->crit.w_orientation;
  return y;
}
// A yardstick taken earlier, on the costmap as it stands now (a list's at each run, tracking's at each step).
BatchYardstick on_costmap(BatchYardstick y, const mppi_ctx* c) {
  y.hw = c->cmap.hw;
  y.res_c = c->cmap.res;
  return y;
}

// The wheel options of a form: each table where `t` turns it on (wlog; wacc; macc and metrics), else null.
BatchWheelOpts wheel_opts(const mppi_batch* b, const WheelTables& t, float* wlog, BatchWheelAcc* wacc,
                          PathMetricsAcc* macc, PathMetrics* metrics) {
  BatchWheelOpts x{};
  x.wlog = t.wlog ? wlog : nullptr;
  x.wacc = t.wacc ? wacc : nullptr;
  x.macc = t.metrics ? macc : nullptr;
  x.metrics = t.metrics ? metrics : nullptr;
  x.off = b->c->p.wheel_offset;
  return x;
}

// One step of the batch on the context's stream: the noise, one rollout launch per projection in use (a
// workgroup of the other projection's episode returns at once; without variants that is the run's
// projection alone), and the finish in the form given.
template <class Form>
int enqueue_step(mppi_batch* b, const RolloutArgs& a, const FinishArgs& f, const BatchArgs& z, const Plan& pl,
                 const bool* use_proj, const Form& finish) {
  mppi_ctx* c = b->c;
  HIP_TRY(launch_batch_noise(z, c->p.k_offset, c->stream, noise_plan(b)));
  for (int pj = MPPI_PROJ_2D; pj <= MPPI_PROJ_3D; ++pj)
    if (use_proj[pj]) HIP_TRY(launch_batch_rollout(a, z, pl.lds_bytes, c->stream, pj));
  HIP_TRY(launch_batch_finish(f, z, finish, pl.fin_lds_bytes, c->stream));
  return MPPI_OK;
}

// Up to n_steps steps while an episode is active, the host reading the pinned count every
// pol.check_every steps; then last_ms takes the stream time since ev[0], which the caller recorded
// ahead of whatever else it times.
template <class Form>
int run_steps(mppi_batch* b, const RolloutArgs& a, const FinishArgs& f, const BatchArgs& z, const Plan& pl,
              const bool* use_proj, const Form& finish, int n_steps, const mppi_loop_policy& pol) {
  mppi_ctx* c = b->c;
  const int every = pol.check_every > 0 ? pol.check_every : 16;
  for (int done = 0; done < n_steps && __atomic_load_n(b->active_count.get(), __ATOMIC_ACQUIRE) > 0;) {
    const int m = std::min(every, n_steps - done);
    for (int i = 0; i < m; ++i)
      if (int rc = enqueue_step(b, a, f, z, pl, use_proj, finish)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    done += m;
  }
  HIP_TRY(hipEventRecord(b->ev[1], c->stream));
  HIP_TRY(hipEventSynchronize(b->ev[1]));
  float ms = 0.f;
  HIP_TRY(hipEventElapsedTime(&ms, b->ev[0], b->ev[1]));
  b->last_ms = ms;
  return MPPI_OK;
}

int batch_run(mppi_batch* b, int proj, int n_steps, const mppi_loop_policy& pol) {
  mppi_ctx* c = b->c;
  const Plan pl = make_plan(c);
  if (!pl.roles || pl.blocks != b->blocks)
    return fail(MPPI_ESTATE, "batch: the context does not run the role-split rollout plan (MPPI_ROLES=0)");
  int rc = batch_pull(b);
  if (rc) return rc;
  int active = 0;
  // the projections in use: a set episode's variant's, or the run's where it holds none
  bool any_var = false, use_proj[4] = {false, false, false, false};
  for (int e = 0; e < b->E; ++e) {
    BatchEpisode& r = b->host[e];
    b->origin[e] = {r.x0, r.y0, r.gx, r.gy};
    if (b->is_set[e]) {
      const int vi = b->ep_var[e];
      any_var = any_var || vi >= 0;
      use_proj[vi >= 0 ? b->variants[vi].proj : proj] = true;
    }
    r.steps_run = 0;
    // (inside on both axes; a NaN coordinate is outside: include/mppi.h)
    const bool outside = !(std::fabs(r.x0 - r.gx) <= pol.goal_tol && std::fabs(r.y0 - r.gy) <= pol.goal_tol);
    r.active = b->is_set[e] && outside ? 1 : 0;
    if (b->is_set[e] && !outside) r.reached = 1;
    active += r.active;
  }
  b->last_ms = 0;
  if (n_steps == 0 || active == 0) {
    HIP_TRY(hipMemcpyAsync(b->ep, b->host.data(), (size_t)b->E * sizeof(BatchEpisode), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return MPPI_OK;
  }
  const size_t log_need = (size_t)b->E * n_steps * 8 * sizeof(float);
  rc = grow(b->log, log_need, c->stream);
  if (rc) return rc;
  BatchWheelBook wb = b->wbook;  // (the book takes the run once its array stands)
  if (wb.take_run().wlog) {      // the parallel array, 24 bytes per log row
    rc = grow(b->wlog, (size_t)b->E * n_steps * 6 * sizeof(float), c->stream);
    if (rc) return rc;
  } else {
    b->wlog.reset();
  }
  b->wbook = wb;
  b->log_cap = n_steps;
  HIP_TRY(hipMemcpyAsync(b->ep, b->host.data(), (size_t)b->E * sizeof(BatchEpisode), hipMemcpyHostToDevice,
                         c->stream));
  __atomic_store_n(b->active_count.get(), active, __ATOMIC_RELEASE);

  RolloutArgs a;
  FinishArgs f;
  step_args(c, pl, a, f);
  BatchArgs z = batch_args(b, proj, pol);
  z.var = any_var ? b->d_var : nullptr;  // null: the kernels of the batch without variants
  z.log = b->log;
  z.log_cap = b->log_cap;
  z.scene = b->book.need_table() ? b->d_tab.get() : nullptr;  // null: the kernels of the batch without scenes
  HIP_TRY(hipEventRecord(b->ev[0], c->stream));
  if (b->wbook.log_wheels()) {  // the wheel log on: the finish form that also stores the contacts
    BatchWheelRun wr{};
    wr.x.wlog = b->wlog;
    return run_steps(b, a, f, z, pl, use_proj, wr, n_steps, pol);
  }
  return run_steps(b, a, f, z, pl, use_proj, BatchPlainRun{}, n_steps, pol);
}

// One step of the set episodes from states in device memory: ingest, noise, a rollout per projection
// in use, the finish's step form.  Enqueues and returns: no wait, no copy, no read of pinned memory.
// Everything the host decides comes from its own bookkeeping (is_set, ep_var, variants, book).
// tracked (mppi_batch_step_tracked): the ingest and the finish are their tracked forms; z, done: the
// step's two optional arrays.
int batch_step_device(mppi_batch* b, int proj, const mppi_batch_io& io_in, bool tracked = false,
                      const float* z_dev = nullptr, int32_t* done_dev = nullptr) {
  mppi_ctx* c = b->c;
  const Plan pl = make_plan(c);
  bool any_set = false, any_var = false, use_proj[4] = {false, false, false, false};
  for (int e = 0; e < b->E; ++e) {
    if (!b->is_set[e]) continue;
    any_set = true;
    const int vi = b->ep_var[e];
    any_var = any_var || vi >= 0;
    use_proj[vi >= 0 ? b->variants[vi].proj : proj] = true;
  }
  if (!any_set) return MPPI_OK;  // no episode takes the step
  RolloutArgs a;
  FinishArgs f;
  step_args(c, pl, a, f);
  // (the step form of the finish reads no policy field: no advance, no goal test)
  BatchArgs z = batch_args(b, proj, mppi_loop_policy{0.0f, 1.0f, 0.0f, 0});
  z.var = any_var ? b->d_var : nullptr;
  z.log = b->log;
  z.log_cap = b->log_cap;
  z.scene = b->book.need_table() ? b->d_tab.get() : nullptr;
  BatchIo io;
  io.states = io_in.states;
  io.mask = io_in.mask;
  io.reset = io_in.reset;
  io.seeds = io_in.seeds;
  io.cmd = io_in.cmd;
  io.plan = io_in.plan;
  b->unwaited = true;
  if (!tracked) {
    HIP_TRY(launch_batch_ingest(z, io, b->d_set, BatchPlainRun{}, c->stream));
    return enqueue_step(b, a, f, z, pl, use_proj, io);
  }
  // the records, the tables and the scene of this step around the caps and the yardstick as taken
  BatchTrack t = b->trk;
  t.rec = b->d_track;
  t.runs = b->d_runs;
  t.results = b->d_runres;
  t.z = z_dev;
  t.done = done_dev;
  t.cm = c->cmap.cm;
  t.cm_size = c->cmap.size;
  t.y = on_costmap(t.y, c);
  t.Z = c->dem.Z;
  t.rows = c->dem.rows;
  t.grid = c->dem.cols;
  t.x_min = c->dem.x_min;
  t.y_min = c->dem.y_min;
  t.res = c->dem.res;
  z.goal_tol = b->trk_goal_tol;
  const WheelTables& wt = b->wbook.tracking();
  if (wt.any()) {
    const BatchWheelTrack w{t, wheel_opts(b, wt, b->wlog, b->d_twacc, b->d_tmacc, b->d_runmetrics)};
    HIP_TRY(launch_batch_ingest(z, io, b->d_set, w, c->stream));
  } else {
    HIP_TRY(launch_batch_ingest(z, io, b->d_set, t, c->stream));
  }
  return enqueue_step(b, a, f, z, pl, use_proj, BatchTrackedIo{io, b->d_track});
}

// The own-model runs and the task queue write the log, steps_last_run and the episode records that a
// tracked run owns.
int tracking_busy(const mppi_batch* b, const char* who) {
  if (!b->tracking) return MPPI_OK;
  return fail(MPPI_ESTATE, std::string(who) + ": tracking is set for the device steps (turn it off with "
                                              "mppi_batch_set_tracking(b, NULL, 0, 0, 0, 0))");
}

// ---- the task queue ----

// An entry point that writes an episode's record or its row of the device's tables, while the
// lanes of an unfinished campaign own them.
int campaign_busy(const mppi_batch* b, const char* who) {
  if (b->campaign != mppi_batch::kUnfinished) return MPPI_OK;
  return fail(MPPI_ESTATE, std::string(who) + ": a campaign is unfinished (go on with mppi_batch_run_tasks, or "
                                              "replace or clear the list with mppi_batch_set_tasks)");
}

// A campaign used the episodes as lanes.  The host puts its own per-episode variant indices and
// scene records back on the device, and every episode is un-set (synchronous).
int campaign_restore(mppi_batch* b) {
  mppi_ctx* c = b->c;
  const size_t E = (size_t)b->E;
  std::vector<SceneRecord> recs(E);
  for (size_t e = 0; e < E; ++e) recs[e] = b->book.record((int)e);
  HIP_TRY(hipMemcpyAsync(b->d_ep_var, b->ep_var.data(), E * sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(b->d_tab->rec, recs.data(), E * sizeof(BatchScene), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(b->ep, 0, E * sizeof(BatchEpisode), c->stream));
  HIP_TRY(hipMemsetAsync(b->d_set, 0, E * sizeof(int), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // recs is pageable and dies here
  b->host.assign(E, BatchEpisode{});
  b->is_set.assign(E, 0);
  b->book.mark_all_unset();
  return MPPI_OK;
}

std::string task_error(const mppi_batch* b, int i, const mppi_batch_task& t, TaskError err, SceneKind kind) {
  const std::string who = "task " + std::to_string(i) + ": ";
  const int32_t s = kind == kSceneDem ? t.dem_slot : t.costmap_slot;
  const std::string slot = std::string(kind == kSceneDem ? "dem_slot " : "costmap_slot ") + std::to_string(s);
  switch (err) {
    case kTaskVariant:
      return who + "variant " + std::to_string(t.variant) + " outside the table of " +
             std::to_string(b->variants.size()) + " rows";
    case kTaskSlotRange:
      return who + slot + " outside [-1, " + std::to_string(b->book.slots(kind)) + ")";
    case kTaskSlotEmpty:
      return who + slot + " is empty";
    case kTaskSlotGeometry:
      return who + slot + " was set with another geometry than the context's current " +
             (kind == kSceneDem ? "DEM" : "costmap");
    case kTaskKRange:
      return who + "num_trajectories " + std::to_string(t.num_trajectories) + " outside [1, " +
             std::to_string(b->c->p.num_trajectories) + "] (0: the context's)";
    case kTaskMaxSteps:
      return who + "max_steps " + std::to_string(t.max_steps) + " must be >= 1";
    default:
      return who + "the caps of the list sum to too many log rows";
  }
}

void task_list_clear(mppi_batch* b) {
  b->tbook.clear();
  b->tasks.clear();
  b->res.clear();
  b->campaign = mppi_batch::kNotStarted;
  b->scored = false;
  b->wbook.clear_list();  // and its tables go with it
  b->twlog.reset();
  b->d_wacc.reset();
  b->d_macc.reset();
  b->d_metrics.reset();
}

BatchCampaign campaign_args(mppi_batch* b) {
  BatchCampaign q{};
  q.tasks = b->d_tasks;
  q.res = b->d_res;
  q.lane = b->d_lane;
  q.next_task = b->d_count;
  q.lane_steps = b->d_count + 1;
  q.log = b->tbook.keeps_log() ? b->tlog.get() : nullptr;
  q.ep_var = b->d_ep_var;
  q.rec = b->d_tab->rec;
  q.n = b->tbook.size();
  return q;
}

// Results, lanes and step counters device -> host; a running task's result is its lane's state.
int campaign_pull(mppi_batch* b) {
  mppi_ctx* c = b->c;
  const size_t E = (size_t)b->E, N = b->res.size();
  std::vector<BatchLane> lanes(E);
  std::vector<int> count(E + 1);
  HIP_TRY(hipMemcpyAsync(b->res.data(), b->d_res, N * sizeof(BatchTaskResult), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(lanes.data(), b->d_lane, E * sizeof(BatchLane), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(count.data(), b->d_count, (E + 1) * sizeof(int), hipMemcpyDeviceToHost, c->stream));
  if (int rc = batch_pull(b)) return rc;  // waits for the stream
  b->lane_steps.assign(count.begin() + 1, count.end());
  for (size_t e = 0; e < E; ++e) {
    const BatchEpisode& r = b->host[e];
    const int i = lanes[e].task;
    if (!r.active || i < 0 || (size_t)i >= N) continue;
    b->res[i] = BatchTaskResult{r.x0, r.y0, r.h0x, r.h0y, r.h0z, r.wl, r.wr, r.gx, r.gy, r.s1, r.s2, r.steps_run, 0, 1};
  }
  return MPPI_OK;
}

int campaign_run(mppi_batch* b, int proj, int n_steps, const mppi_loop_policy& pol, int32_t* tasks_done,
                 int64_t* batch_steps) {
  mppi_ctx* c = b->c;
  const int N = b->tbook.size();
  auto report = [&](int64_t steps) {
    int done = 0;
    for (const BatchTaskResult& r : b->res) done += (r.flags & 2) ? 1 : 0;
    if (tasks_done) *tasks_done = done;
    if (batch_steps) *batch_steps = steps;
  };
  b->last_ms = 0;
  if (b->campaign == mppi_batch::kComplete) {
    report(0);
    return MPPI_OK;
  }
  const Plan pl = make_plan(c);
  if (!pl.roles || pl.blocks != b->blocks)
    return fail(MPPI_ESTATE, "batch: the context does not run the role-split rollout plan (MPPI_ROLES=0)");
  RolloutArgs a;
  FinishArgs f;
  step_args(c, pl, a, f);
  BatchArgs z = batch_args(b, proj, pol);
  // the tables and the projections are decided from the list: the lanes' own rows change as they claim
  z.var = b->tbook.need_variants() ? b->d_var.get() : nullptr;
  z.scene = b->tbook.need_scene() ? b->d_tab.get() : nullptr;
  std::vector<int> vproj(b->variants.size());
  for (size_t i = 0; i < vproj.size(); ++i) vproj[i] = b->variants[i].proj;
  bool use_proj[4];
  b->tbook.projections(vproj, proj, use_proj);
  const BatchCampaign q = campaign_args(b);
  const size_t E = (size_t)b->E;
  // a scored list: the queue, the tables and the yardstick of the list on the costmap of this run
  const BatchScoredCampaign sq{q, b->d_acc, b->d_score, c->cmap.cm, c->cmap.size, on_costmap(b->yard, c)};
  // a list set with the wheel log, the wheel slope mode or the metrics on: the wheel forms of the finish
  const WheelTables& lt = b->wbook.list();
  const BatchWheelOpts wx = wheel_opts(b, lt, b->twlog, b->d_wacc, b->d_macc, b->d_metrics);
  HIP_TRY(hipEventRecord(b->ev[0], c->stream));
  if (b->campaign == mppi_batch::kNotStarted) {
    // the first fill: every lane empty and counted active, then one claim each
    HIP_TRY(hipMemsetAsync(b->ep, 0, E * sizeof(BatchEpisode), c->stream));
    HIP_TRY(hipMemsetAsync(b->d_res, 0, (size_t)N * sizeof(BatchTaskResult), c->stream));
    HIP_TRY(hipMemsetAsync(b->d_count, 0, (E + 1) * sizeof(int), c->stream));
    HIP_TRY(hipMemsetAsync(b->d_lane, 0xff, E * sizeof(BatchLane), c->stream));
    __atomic_store_n(b->active_count.get(), b->E, __ATOMIC_RELEASE);
    b->lane_steps.assign(E, 0);
    b->campaign = mppi_batch::kUnfinished;
    if (b->scored) {  // no task has a score yet; the claim resets the lanes' records
      HIP_TRY(hipMemsetAsync(b->d_score, 0, (size_t)N * sizeof(BatchTaskScore), c->stream));
      HIP_TRY(hipMemsetAsync(b->d_acc, 0, E * sizeof(BatchScoreAcc), c->stream));
      if (lt.wacc) HIP_TRY(hipMemsetAsync(b->d_wacc, 0, E * sizeof(BatchWheelAcc), c->stream));
      if (lt.metrics) {
        HIP_TRY(hipMemsetAsync(b->d_macc, 0, E * sizeof(PathMetricsAcc), c->stream));
        HIP_TRY(hipMemsetAsync(b->d_metrics, 0, (size_t)N * sizeof(PathMetrics), c->stream));
      }
      HIP_TRY(launch_batch_claim(z, sq, c->stream));
    } else {
      HIP_TRY(launch_batch_claim(z, q, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  const int before = *std::max_element(b->lane_steps.begin(), b->lane_steps.end());
  int rc;
  if (lt.any() && b->scored) rc = run_steps(b, a, f, z, pl, use_proj, BatchWheelScored{sq, wx}, n_steps, pol);
  else if (lt.any()) rc = run_steps(b, a, f, z, pl, use_proj, BatchWheelCampaign{q, wx}, n_steps, pol);
  else if (b->scored) rc = run_steps(b, a, f, z, pl, use_proj, sq, n_steps, pol);
  else rc = run_steps(b, a, f, z, pl, use_proj, q, n_steps, pol);
  if (rc) return rc;
  if ((rc = campaign_pull(b))) return rc;
  report((int64_t)*std::max_element(b->lane_steps.begin(), b->lane_steps.end()) - before);
  if (__atomic_load_n(b->active_count.get(), __ATOMIC_ACQUIRE) <= 0) {
    b->campaign = mppi_batch::kComplete;
    return campaign_restore(b);
  }
  return MPPI_OK;
}

// One launch of the log scorer over E paths of `log` (goals [E]; cmaps [E] or empty: every path on the
// context's costmap; base_rows [E] or empty: path p begins at row p * stride), the results to the host.
int score_logs(mppi_batch* b, const std::vector<ScoreGoal>& goals, const std::vector<const float*>& cmaps,
               const std::vector<int64_t>& base_rows, const float* log, const int32_t* lengths, int len_step,
               int stride, const mppi_batch_variant* yardstick, mppi_path_scores* out, int32_t* rows,
               const char* who, const float* wlog = nullptr, mppi_path_metrics* metrics = nullptr) {
  mppi_ctx* c = b->c;
  const size_t E = goals.size();
  // one allocation, every array 16-byte aligned: [goals][cost][terms][collisions][rows][costmaps][base rows]
  // (wlog: the wheel log beside `log`, the slope term in its wheel form; metrics: [E] host rows, the path
  // metrics of each log, a second small launch), then [metrics]
  const size_t bg = up16(E * sizeof(ScoreGoal)), bn = up16(E * 4), bt = E * 16, bp = up16(cmaps.size() * sizeof(float*)),
               bb = up16(base_rows.size() * sizeof(int64_t)), bm = metrics ? E * sizeof(PathMetrics) : 0;
  DeviceBuf<char> dbuf;
  HIP_TRY(dbuf.alloc(bg + bn * 3 + bt + bp + bb + bm));
  char* buf = dbuf;
  ScoreGoal* d_goals = (ScoreGoal*)buf;
  float* d_cost = (float*)(buf + bg);
  float* d_terms = (float*)(buf + bg + bn);
  int32_t* d_col = (int32_t*)(buf + bg + bn + bt);
  int32_t* d_rows = (int32_t*)(buf + bg + bn + bt + bn);
  const float** d_cmaps = (const float**)(buf + bg + bn + bt + bn + bn);
  int64_t* d_base = (int64_t*)(buf + bg + bn + bt + bn + bn + bp);
  PathMetrics* d_met = (PathMetrics*)(buf + bg + bn + bt + bn + bn + bp + bb);
  ScoreArgs a;
  std::memset(&a, 0, sizeof(a));
  a.log = log;
  a.lw = wlog;
  a.goals = d_goals;
  a.lengths = lengths;  // the device table's own counters, len_step ints apart
  a.len_step = len_step;
  a.rows_out = d_rows;
  a.n = (int64_t)E;
  a.stride = stride;
  const BatchYardstick y = resolve_yardstick(c, yardstick);  // (w_orient: the context's set; a log is a body
  a.cm = c->cmap.cm;                                         // path in either slope mode)
  a.cm_size = c->cmap.size;
  a.hw = y.hw;
  a.res_c = y.res_c;
  a.vmax = y.vmax;
  a.thr = y.thr;
  a.pen = y.pen;
  a.w_path = y.w_path;
  a.w_slope = y.w_slope;
  a.w_speed = y.w_speed;
  a.w_obs = y.w_obs;
  a.w_orient = y.w_orient;
  a.cost = d_cost;
  a.terms = d_terms;
  a.collisions = d_col;
  a.cm_path = bp ? d_cmaps : nullptr;
  a.base_row = bb ? d_base : nullptr;
  hipError_t e = hipMemcpyAsync(d_goals, goals.data(), E * sizeof(ScoreGoal), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && bp)
    e = hipMemcpyAsync(d_cmaps, cmaps.data(), cmaps.size() * sizeof(float*), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && bb)
    e = hipMemcpyAsync(d_base, base_rows.data(), base_rows.size() * sizeof(int64_t), hipMemcpyHostToDevice, c->stream);
  int rc = MPPI_OK;
  if (e == hipSuccess) rc = run_score(c, a);
  if (e == hipSuccess && rc == MPPI_OK && metrics) {
    e = launch_log_metrics(log, lengths, len_step, a.base_row, stride, (int64_t)E, d_met, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(metrics, d_met, bm, hipMemcpyDeviceToHost, c->stream);
  }
  if (e == hipSuccess && rc == MPPI_OK && out->cost) e = hipMemcpyAsync(out->cost, d_cost, E * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == MPPI_OK && out->terms) e = hipMemcpyAsync(out->terms, d_terms, E * 16, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == MPPI_OK && out->collisions) e = hipMemcpyAsync(out->collisions, d_col, E * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess && rc == MPPI_OK && rows) e = hipMemcpyAsync(rows, d_rows, E * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  if (e != hipSuccess) return fail(MPPI_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  return MPPI_OK;
}

}  // namespace

extern "C" {

int mppi_batch_create(mppi_ctx* c, int32_t episodes, mppi_batch** out) {
  if (!out) return fail(MPPI_EINVAL, "null argument");
  *out = nullptr;
  if (episodes < 1 || episodes > 4096) return fail(MPPI_EINVAL, "episodes must be in [1, 4096]");
  if (!c) return fail(MPPI_EINVAL, "null context");
  const int64_t K = c->p.num_trajectories;
  const int64_t blocks = (K + PAIR_TRAJ - 1) / PAIR_TRAJ;
  if (blocks < 1 || blocks > kBatchMaxRecords)
    return fail(MPPI_EINVAL, "batch: num_trajectories must be in [1, 4096] (1 to 16 leaf records)");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  std::unique_ptr<mppi_batch> b(new mppi_batch());
  b->c = c;
  b->E = episodes;
  b->blocks = (int)blocks;
  const int H = b->H = H_of(c);
  const size_t E = (size_t)episodes;
  b->host.assign(E, BatchEpisode{});
  b->is_set.assign(E, 0);
  b->ep_var.assign(E, -1);
  b->origin.assign(E, std::array<float, 4>{0.0f, 0.0f, 0.0f, 0.0f});
  b->book = BatchSceneBook(episodes, kBatchMaxDems, kBatchMaxCostmaps, K);
  b->dems.resize(kBatchMaxDems);
  b->cms.resize(kBatchMaxCostmaps);
  std::vector<SceneRecord> recs(E);
  for (size_t e = 0; e < E; ++e) recs[e] = b->book.record((int)e);
  const size_t tab_bytes = offsetof(BatchSceneTable, rec) + E * sizeof(BatchScene);
  if (b->ep.alloc(E * sizeof(BatchEpisode)) || b->d_var.alloc(kBatchMaxVariants * sizeof(BatchVariant)) ||
      b->d_ep_var.alloc(E * sizeof(int)) || b->d_tab.alloc(tab_bytes) || b->d_set.alloc(E * sizeof(int)) ||
      hipMemset(b->d_set, 0, E * sizeof(int)) != hipSuccess ||
      hipMemset(b->d_tab, 0, tab_bytes) != hipSuccess ||
      hipMemcpy(b->d_tab->rec, recs.data(), E * sizeof(BatchScene), hipMemcpyHostToDevice) != hipSuccess ||
      hipMemset(b->d_var, 0, kBatchMaxVariants * sizeof(BatchVariant)) != hipSuccess ||
      hipMemset(b->d_ep_var, 0xff, E * sizeof(int)) != hipSuccess ||
      b->eps.alloc(E * blocks * 2 * H * 256 * sizeof(float)) || b->unom.alloc(E * 4 * H * sizeof(float)) ||
      b->nodes.alloc(E * blocks * (2 * H + 2) * sizeof(double)) || b->cost.alloc(E * blocks * 256 * sizeof(float)) ||
      b->fin.alloc(E * (7 * H + 12) * sizeof(float)) || b->active_count.alloc(64) || b->ev[0].create() ||
      b->ev[1].create() ||
      hipMemset(b->ep, 0, E * sizeof(BatchEpisode)) != hipSuccess ||
      hipMemset(b->unom, 0, E * 4 * H * sizeof(float)) != hipSuccess ||
      hipMemset(b->cost, 0, E * blocks * 256 * sizeof(float)) != hipSuccess ||
      hipMemset(b->fin, 0, E * (7 * H + 12) * sizeof(float)) != hipSuccess ||
      hipDeviceSynchronize() != hipSuccess) {
    const std::string why = hipGetErrorString(hipGetLastError());
    return fail(MPPI_EHIP, "batch allocation failed: " + why);
  }
  *b->active_count = 0;
  *out = b.release();
  return MPPI_OK;
}

void mppi_batch_destroy(mppi_batch* b) {
  if (!b) return;
  hipSetDevice(b->c->device);
  if (b->c->stream) hipStreamSynchronize(b->c->stream);
  delete b;
}

int mppi_batch_set_episode(mppi_batch* b, int32_t e, const mppi_state* start, uint64_t seed) {
  if (int rc = batch_episode(b, e)) return rc;
  if (!start) return fail(MPPI_EINVAL, "null argument");
  if (int rc = campaign_busy(b, "batch_set_episode")) return rc;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  ServerCmd d;
  state_fields(c->p, *start, d);
  BatchEpisode r{};
  r.x0 = d.x0;
  r.y0 = d.y0;
  r.h0x = d.h0x;
  r.h0y = d.h0y;
  r.h0z = d.h0z;
  r.wl = d.wl;
  r.wr = d.wr;
  r.gx = d.gx;
  r.gy = d.gy;
  r.s1 = d.s1;
  r.s2 = d.s2;
  r.pf_far = d.pf_far;
  r.speed_on = d.speed_on;
  r.igx = d.igx;
  r.igy = d.igy;
  r.pf_scale = d.pf_scale;
  r.seed = seed;
  b->host[e] = r;
  b->is_set[e] = 1;
  b->book.mark_set(e);
  HIP_TRY(hipMemcpyAsync(b->ep + e, &b->host[e], sizeof(BatchEpisode), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(b->unom + (size_t)e * 4 * b->H, 0, (size_t)4 * b->H * sizeof(float), c->stream));
  HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)(b->d_set + e), 1, 1, c->stream));
  BatchTrackRec fresh{};  // tracking: the episode's run begins at its next ingest; an unfinished one leaves no result
  fresh.fresh = 1;
  if (b->tracking)
    HIP_TRY(hipMemcpyAsync(b->d_track + e, &fresh, sizeof(fresh), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_batch_run(mppi_batch* b, int32_t proj, int32_t n_steps, const mppi_loop_policy* policy) {
  if (!b || !policy) return fail(MPPI_EINVAL, "null argument");
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  if (n_steps < 0) return fail(MPPI_EINVAL, "n_steps must be >= 0");
  if (policy->check_every < 0) return fail(MPPI_EINVAL, "check_every must be >= 0");
  if (!(policy->sigma_div != 0.0f)) return fail(MPPI_EINVAL, "sigma_div must be non-zero");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (int rc = campaign_busy(b, "batch_run")) return rc;
  if (int rc = tracking_busy(b, "batch_run")) return rc;
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM: call mppi_set_dem first");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "no costmap: call mppi_set_costmap first");
  if (int rc_g = scene_geometry(b)) return rc_g;
  HIP_TRY(hipSetDevice(c->device));
  const int rc = batch_run(b, proj, n_steps, *policy);
  if (rc == MPPI_EHIP) b->failed = true;
  return rc;
}

// mppi_batch_step_device and mppi_batch_step_tracked: one set of refusals.
static int step_entry(mppi_batch* b, int32_t proj, const mppi_batch_io* io, const char* who, bool tracked,
                      const float* z_dev, int32_t* done_dev) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (!io) return fail(MPPI_EINVAL, std::string(who) + ": null io");
  if (!io->states) return fail(MPPI_EINVAL, std::string(who) + ": null states");
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;  // (a host wait only while a resident server is running)
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (int rc = campaign_busy(b, who)) return rc;
  if (tracked && !b->tracking)
    return fail(MPPI_ESTATE, std::string(who) + ": tracking is not set: call mppi_batch_set_tracking first");
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM: call mppi_set_dem first");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "no costmap: call mppi_set_costmap first");
  if (int rc_g = scene_geometry(b)) return rc_g;
  const Plan pl = make_plan(c);
  if (!pl.roles || pl.blocks != b->blocks)
    return fail(MPPI_ESTATE, "batch: the context does not run the role-split rollout plan (MPPI_ROLES=0)");
  HIP_TRY(hipSetDevice(c->device));
  const int rc = batch_step_device(b, proj, *io, tracked, z_dev, done_dev);
  if (rc == MPPI_EHIP) b->failed = true;
  return rc;
}

int mppi_batch_step_device(mppi_batch* b, int32_t proj, const mppi_batch_io* io) {
  return step_entry(b, proj, io, "batch_step_device", false, nullptr, nullptr);
}

int mppi_batch_step_tracked(mppi_batch* b, int32_t proj, const mppi_batch_io* io, const float* z_dev,
                            int32_t* done_dev) {
  return step_entry(b, proj, io, "batch_step_tracked", true, z_dev, done_dev);
}

static int after_wait(mppi_batch* b, int rc);

int mppi_batch_set_tracking(mppi_batch* b, const mppi_batch_variant* yardstick, float goal_tol, int32_t max_steps,
                            int32_t runs_per_episode, int32_t keep_log) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (max_steps < 0) return fail(MPPI_EINVAL, "batch_set_tracking: max_steps must be >= 0 (0 turns tracking off)");
  if (max_steps > 0 && runs_per_episode < 1)
    return fail(MPPI_EINVAL, "batch_set_tracking: runs_per_episode must be >= 1");
  if (max_steps > 0 && !(goal_tol >= 0.0f)) return fail(MPPI_EINVAL, "batch_set_tracking: goal_tol must be >= 0");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (int rc = campaign_busy(b, "batch_set_tracking")) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));  // device steps in flight read the tables
  b->tracking = false;
  b->wbook.clear_tracking();
  b->d_twacc.reset();
  b->d_tmacc.reset();
  b->d_runmetrics.reset();
  if (max_steps == 0) {
    b->d_track.reset();
    b->d_runs.reset();
    b->d_runres.reset();
    return MPPI_OK;
  }
  // the options as they stand (mppi_batch_set_wheel_log / _set_score_options): tables only for those on
  BatchWheelBook wb = b->wbook;  // (the book takes tracking once the tables stand)
  const WheelTables wt = wb.take_tracking(keep_log != 0);
  const bool wheels_log = wt.wlog, slope_wheels = wt.wacc, metrics = wt.metrics;
  const size_t E = (size_t)b->E;
  const size_t res_bytes = E * (size_t)runs_per_episode * sizeof(BatchRunResult);
  const size_t log_bytes = keep_log ? E * (size_t)max_steps * 8 * sizeof(float) : 0;
  if (b->d_track.grow(E * sizeof(BatchTrackRec)) || b->d_runs.grow(E * sizeof(int)) || b->d_runres.grow(res_bytes) ||
      (keep_log && b->log.grow(log_bytes)) || (wheels_log && b->wlog.grow(E * (size_t)max_steps * 6 * sizeof(float))) ||
      (slope_wheels && b->d_twacc.grow(E * sizeof(BatchWheelAcc))) ||
      (metrics && (b->d_tmacc.grow(E * sizeof(PathMetricsAcc)) ||
                   b->d_runmetrics.grow(E * (size_t)runs_per_episode * sizeof(PathMetrics))))) {
    (void)hipGetLastError();
    b->d_track.reset();
    b->d_runs.reset();
    b->d_runres.reset();
    b->d_twacc.reset();
    b->d_tmacc.reset();
    b->d_runmetrics.reset();
    return fail(MPPI_EHIP, "batch_set_tracking: allocation of " + std::to_string(res_bytes) +
                               " bytes of run results and " + std::to_string(log_bytes) + " bytes of log failed");
  }
  b->wbook = wb;          // the tables stand
  BatchTrackRec fresh{};  // every episode's run begins at its next ingest
  fresh.fresh = 1;
  const std::vector<BatchTrackRec> recs(E, fresh);
  HIP_TRY(hipMemcpyAsync(b->d_track, recs.data(), E * sizeof(BatchTrackRec), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(b->d_runs, 0, E * sizeof(int), c->stream));
  HIP_TRY(hipMemsetAsync(b->d_runres, 0, res_bytes, c->stream));
  if (slope_wheels) HIP_TRY(hipMemsetAsync(b->d_twacc, 0, E * sizeof(BatchWheelAcc), c->stream));
  if (metrics) {
    HIP_TRY(hipMemsetAsync(b->d_tmacc, 0, E * sizeof(PathMetricsAcc), c->stream));
    HIP_TRY(hipMemsetAsync(b->d_runmetrics, 0, E * (size_t)runs_per_episode * sizeof(PathMetrics), c->stream));
  }
  if (keep_log) {  // the log is laid out for max_steps rows per episode from here on: no episode has a row
    if (!wheels_log) b->wlog.reset();
    b->log_cap = max_steps;
    HIP_TRY(hipMemset2DAsync(&b->ep->steps_run, sizeof(BatchEpisode), 0, sizeof(int), E, c->stream));
    for (BatchEpisode& r : b->host) r.steps_run = 0;
  }
  HIP_TRY(hipStreamSynchronize(c->stream));  // recs is pageable and dies here
  BatchTrack& t = b->trk;
  t = BatchTrack{};
  t.max_steps = max_steps;
  t.runs_per_episode = runs_per_episode;
  t.keep_log = keep_log ? 1 : 0;
  t.y = resolve_yardstick(c, yardstick);  // the yardstick is taken here, as a scored list takes it
  b->trk_goal_tol = goal_tol;
  b->tracking = true;
  return MPPI_OK;
}

int mppi_batch_get_run_counts(mppi_batch* b, int32_t* counts) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (!counts) return fail(MPPI_EINVAL, "null argument");
  if (!b->tracking)
    return fail(MPPI_ESTATE, "batch_get_run_counts: tracking is not set: call mppi_batch_set_tracking first");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  static_assert(sizeof(int32_t) == sizeof(int), "run counts are int32");
  hipError_t e = hipMemcpyAsync(counts, b->d_runs, (size_t)b->E * sizeof(int), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return after_wait(b, fail(MPPI_EHIP, std::string("batch_get_run_counts: ") + hipGetErrorString(e)));
  return after_wait(b, MPPI_OK);
}

int mppi_batch_get_runs(mppi_batch* b, int32_t e, int32_t first, int32_t count, mppi_state* states, int32_t* steps,
                        int32_t* reached, int32_t* status, mppi_path_scores* out, int32_t* rows, double* length) {
  if (int rc = batch_episode(b, e)) return rc;
  if (!b->tracking) return fail(MPPI_ESTATE, "batch_get_runs: tracking is not set: call mppi_batch_set_tracking first");
  const int R = b->trk.runs_per_episode;
  if (first < 0 || count < 0 || (int64_t)first + count > R)
    return fail(MPPI_EINVAL, "batch_get_runs: runs [" + std::to_string(first) + ", " +
                                 std::to_string((int64_t)first + count) + ") outside the " + std::to_string(R) +
                                 " result rows of an episode");
  if (count == 0) return MPPI_OK;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<BatchRunResult> res((size_t)count);
  hipError_t he = hipMemcpyAsync(res.data(), b->d_runres + ((size_t)e * R + first), (size_t)count * sizeof(BatchRunResult),
                                 hipMemcpyDeviceToHost, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he != hipSuccess) return after_wait(b, fail(MPPI_EHIP, std::string("batch_get_runs: ") + hipGetErrorString(he)));
  for (int32_t i = 0; i < count; ++i) {
    const BatchTaskResult& r = res[(size_t)i].r;
    const BatchTaskScore& s = res[(size_t)i].s;
    if (states) {
      mppi_state& st = states[i];
      st.x = r.x0;
      st.y = r.y0;
      st.heading[0] = r.h0x;
      st.heading[1] = r.h0y;
      st.heading[2] = r.h0z;
      st.left_wheel_speed = r.wl;
      st.right_wheel_speed = r.wr;
      st.goal_x = r.gx;
      st.goal_y = r.gy;
      st.std_dev_u1 = r.s1;
      st.std_dev_u2 = r.s2;
    }
    if (steps) steps[i] = r.steps;
    if (reached) reached[i] = r.reached;
    if (status) status[i] = r.flags;
    if (out && out->cost) out->cost[i] = s.cost;
    if (out && out->terms) std::memcpy(out->terms + 4 * (size_t)i, s.terms, sizeof(s.terms));
    if (out && out->collisions) out->collisions[i] = s.collisions;
    if (rows) rows[i] = s.rows;
    if (length) length[i] = s.length;
  }
  return after_wait(b, MPPI_OK);
}

// The two readers below wait for the stream: a HIP error of steps that mppi_batch_step_device
// enqueued surfaces in them, and refuses the batch as a failed run does.
static int after_wait(mppi_batch* b, int rc) {
  if (rc == MPPI_EHIP && b->unwaited) b->failed = true;
  if (rc == MPPI_OK) b->unwaited = false;
  return rc;
}
static int get_episode(mppi_batch* b, int32_t e, mppi_state* state, int64_t* steps_total, int32_t* steps_last_run,
                       int32_t* reached, float* u1, float* u2);
static int get_log(mppi_batch* b, int32_t e, int32_t first, int32_t count, float* rows);

int mppi_batch_get_episode(mppi_batch* b, int32_t e, mppi_state* state, int64_t* steps_total,
                           int32_t* steps_last_run, int32_t* reached, float* u1, float* u2) {
  if (int rc = batch_episode(b, e)) return rc;
  return after_wait(b, get_episode(b, e, state, steps_total, steps_last_run, reached, u1, u2));
}

int mppi_batch_get_log(mppi_batch* b, int32_t e, int32_t first, int32_t count, float* rows) {
  if (int rc = batch_episode(b, e)) return rc;
  if (first < 0 || count < 0) return fail(MPPI_EINVAL, "log range out of bounds");
  if (count > 0 && !rows) return fail(MPPI_EINVAL, "null argument");
  return after_wait(b, get_log(b, e, first, count, rows));
}

static int get_episode(mppi_batch* b, int32_t e, mppi_state* state, int64_t* steps_total, int32_t* steps_last_run,
                       int32_t* reached, float* u1, float* u2) {
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  BatchEpisode& r = b->host[e];
  const int H = b->H;
  HIP_TRY(hipMemcpyAsync(&r, b->ep + e, sizeof(BatchEpisode), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const float* unom = b->unom + ((size_t)e * 2 + r.cur) * 2 * H;
  if (u1) HIP_TRY(hipMemcpyAsync(u1, unom, H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (u2) HIP_TRY(hipMemcpyAsync(u2, unom + H, H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (u1 || u2) HIP_TRY(hipStreamSynchronize(c->stream));
  if (state) {
    state->x = r.x0;
    state->y = r.y0;
    state->heading[0] = r.h0x;
    state->heading[1] = r.h0y;
    state->heading[2] = r.h0z;
    state->left_wheel_speed = r.wl;
    state->right_wheel_speed = r.wr;
    state->goal_x = r.gx;
    state->goal_y = r.gy;
    state->std_dev_u1 = r.s1;
    state->std_dev_u2 = r.s2;
  }
  if (steps_total) *steps_total = (int64_t)r.step;
  if (steps_last_run) *steps_last_run = r.steps_run;
  if (reached) *reached = r.reached;
  return MPPI_OK;
}

static int get_log(mppi_batch* b, int32_t e, int32_t first, int32_t count, float* rows) {
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  BatchEpisode& r = b->host[e];
  HIP_TRY(hipMemcpyAsync(&r, b->ep + e, sizeof(BatchEpisode), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if ((int64_t)first + count > r.steps_run) return fail(MPPI_EINVAL, "log range beyond the steps of the last run");
  if (count == 0) return MPPI_OK;
  HIP_TRY(hipMemcpyAsync(rows, b->log + ((size_t)e * b->log_cap + first) * 8, (size_t)count * 8 * sizeof(float),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_batch_get_ms(mppi_batch* b, double* ms) {
  if (!b || !ms) return fail(MPPI_EINVAL, "null argument");
  *ms = b->last_ms;
  return MPPI_OK;
}

int mppi_batch_variant_default(mppi_batch* b, int32_t proj, const mppi_loop_policy* policy,
                               mppi_batch_variant* out) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (!policy || !out) return fail(MPPI_EINVAL, "null argument");
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  const mppi_params& p = b->c->p;
  out->w_path = p.w_path;
  out->w_slope = p.w_slope;
  out->w_speed = p.w_speed;
  out->w_obstacle = p.w_obstacle;
  out->collision_threshold = p.collision_threshold;
  out->collision_penalty = p.collision_penalty;
  out->temperature = p.temperature;
  out->filter_k = p.filter_k;
  out->filter_a = p.filter_a;
  out->opt_filter_k = p.opt_filter_k;
  out->opt_filter_a = p.opt_filter_a;
  out->sigma_base = policy->sigma_base;
  out->sigma_div = policy->sigma_div;
  out->proj = proj;
  return MPPI_OK;
}

int mppi_batch_set_variants(mppi_batch* b, int32_t n, const mppi_batch_variant* v) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (n < 0 || n > kBatchMaxVariants) return fail(MPPI_EINVAL, "variants: n must be in [0, 1024]");
  if (n > 0 && !v) return fail(MPPI_EINVAL, "null argument");
  for (int i = 0; i < n; ++i) {
    const std::string row = "variant row " + std::to_string(i) + ": ";
    // the checks of mppi_create on the fields a variant overrides, and the run's on sigma_div / proj
    if (!(v[i].temperature > 0.0f)) return fail(MPPI_EINVAL, row + "temperature must be > 0");
    if (!(v[i].sigma_div != 0.0f)) return fail(MPPI_EINVAL, row + "sigma_div must be non-zero");
    if (v[i].proj != MPPI_PROJ_2D && v[i].proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, row + "proj must be 2 or 3");
  }
  for (int e = 0; e < b->E; ++e)
    if (b->ep_var[e] >= n)
      return fail(MPPI_EINVAL, "variants: episode " + std::to_string(e) + " holds row " +
                                   std::to_string(b->ep_var[e]) + " of the table, n = " + std::to_string(n));
  if (const int i = b->tbook.variant_beyond(n); i >= 0)
    return fail(MPPI_EINVAL, "variants: task " + std::to_string(i) + " of the task list holds row " +
                                 std::to_string(b->tbook.task(i).variant) + " of the table, n = " + std::to_string(n));
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<BatchVariant> rows((size_t)n);
  for (int i = 0; i < n; ++i) rows[i] = device_variant(v[i]);
  if (n > 0) {
    HIP_TRY(hipMemcpyAsync(b->d_var, rows.data(), (size_t)n * sizeof(BatchVariant), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));  // rows is pageable and dies here
  }
  b->variants.assign(v, v + n);
  return MPPI_OK;
}

int mppi_batch_set_variant_critics(mppi_batch* b, int32_t n, const mppi_critics* rows) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (n < 0 || n > kBatchMaxVariants)
    return fail(MPPI_EINVAL, "batch: need 0 <= n <= " + std::to_string(kBatchMaxVariants) + " critic rows");
  if (n > 0 && !rows) return fail(MPPI_EINVAL, "null argument");
  for (int i = 0; i < n; ++i) {
    const std::string err = critics_error(rows[i], b->H);
    if (!err.empty()) return fail(MPPI_EINVAL, "batch: critic row " + std::to_string(i) + ": " + err);
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (no run of the batch is in flight: every call waits)
  if (n > 0) {
    if (!b->d_crit && b->d_crit.alloc(kBatchMaxVariants * sizeof(BatchCriticRow)))
      return fail(MPPI_EHIP, "batch: critic table allocation failed");
    std::vector<BatchCriticRow> tab(kBatchMaxVariants, BatchCriticRow{-1, 0.0f});
    for (int i = 0; i < n; ++i) tab[i] = BatchCriticRow{rows[i].slope_mode, rows[i].w_orientation};
    HIP_TRY(hipMemcpyAsync(b->d_crit, tab.data(), tab.size() * sizeof(BatchCriticRow), hipMemcpyHostToDevice,
                           c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  b->critics.assign(rows, rows + n);
  return MPPI_OK;
}

int mppi_batch_set_variant_sampling(mppi_batch* b, int32_t n, const mppi_sampling* rows) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (n < 0 || n > kBatchMaxVariants)
    return fail(MPPI_EINVAL, "batch: need 0 <= n <= " + std::to_string(kBatchMaxVariants) + " sampling rows");
  if (n > 0 && !rows) return fail(MPPI_EINVAL, "null argument");
  for (int i = 0; i < n; ++i) {
    const std::string err = sampling_error(rows[i], c->p.k_offset);
    if (!err.empty()) return fail(MPPI_EINVAL, "batch: sampling row " + std::to_string(i) + ": " + err);
  }
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (no run of the batch is in flight: every call waits)
  if (n > 0) {
    if (!b->d_samp && b->d_samp.alloc(kBatchMaxVariants * sizeof(SamplePlan)))
      return fail(MPPI_EHIP, "batch: sampling table allocation failed");
    std::vector<SamplePlan> tab(kBatchMaxVariants, SamplePlan{-1, 0, 0.0f, 1.0f});
    for (int i = 0; i < n; ++i) tab[i] = device_plan(rows[i]);
    HIP_TRY(hipMemcpyAsync(b->d_samp, tab.data(), tab.size() * sizeof(SamplePlan), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  b->sampling.assign(rows, rows + n);
  return MPPI_OK;
}

int mppi_batch_set_episode_variant(mppi_batch* b, int32_t e, int32_t variant) {
  if (int rc = batch_episode(b, e)) return rc;
  if (variant < -1 || variant >= (int32_t)b->variants.size())
    return fail(MPPI_EINVAL, "variant index " + std::to_string(variant) + " outside the table of " +
                                 std::to_string(b->variants.size()) + " rows");
  if (int rc = campaign_busy(b, "batch_set_episode_variant")) return rc;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  b->ep_var[e] = variant;
  HIP_TRY(hipMemcpyAsync(b->d_ep_var + e, &b->ep_var[e], sizeof(int), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_batch_set_dem(mppi_batch* b, int32_t slot, const float* z_host) {
  if (int rc = slot_index(b, kSceneDem, slot)) return rc;
  mppi_ctx* c = b->c;
  if (!z_host) {
    if (int rc_q = quiesce(c)) return rc_q;
    HIP_TRY(hipSetDevice(c->device));
    return slot_free(b, kSceneDem, slot);
  }
  return batch_fill_dem(b, slot, "batch_set_dem", [&](float* dst) {
    HIP_TRY(hipMemcpyAsync(dst, z_host, (size_t)c->dem.rows * c->dem.cols * sizeof(float), hipMemcpyHostToDevice,
                           c->stream));
    return (int)MPPI_OK;
  });
}

// What mppi_capi_dem.cpp needs of a batch, whose layout stays in this file.
extern "C++" mppi_ctx* mppi::capi::batch_context(mppi_batch* b) { return b->c; }
extern "C++" int mppi::capi::batch_dem_slot(const mppi_batch* b, int32_t slot) { return slot_index(b, kSceneDem, slot); }

// mppi_batch_set_dem for heights that `fill(dst)` enqueues on the context stream into the slot's
// buffer (the copy from the host, or mppi_batch_build_dem's product kernel); slot is in range.
extern "C++" int mppi::capi::batch_fill_dem(mppi_batch* b, int32_t slot, const char* who,
                                            const std::function<int(float*)>& fill) {
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  if (!c->dem.Z || c->dem.rows <= 0)
    return fail(MPPI_ESTATE, std::string(who) + ": no DEM: call mppi_set_dem first (a slot takes the context's geometry)");
  const int rows = c->dem.rows, cols = c->dem.cols;
  const size_t zb = (size_t)rows * cols * sizeof(float);
  const size_t nb = ((size_t)rows + 1) * ((size_t)cols + 1) * sizeof(float4);
  Dem& d = b->dems[slot];
  DeviceBuf<float> nz;
  DeviceBuf<float4> nt;
  if (int rc = slot_alloc(d.Z, nz, zb, "DEM", slot)) return rc;
  if (int rc = slot_alloc(d.ntab, nt, nb, "DEM", slot)) return rc;
  // (filled before a new buffer replaces the slot's: a fill that fails leaves a live slot's buffers in place)
  if (int rc = fill(nz ? nz.get() : d.Z.get())) return rc;
  if (nz) d.Z = std::move(nz);
  if (nt) d.ntab = std::move(nt);
  d.rows = rows;
  d.cols = cols;
  d.x_min = c->dem.x_min;
  d.y_min = c->dem.y_min;
  d.res = c->dem.res;
  d.rinv_res = c->dem.rinv_res;
  const float* zp = d.Z;
  const float4* np = d.ntab;
  HIP_TRY(launch_normal_table(d.Z, rows, cols, d.res, d.ntab, c->stream));
  HIP_TRY(hipMemcpyAsync(b->d_tab->dem_z + slot, &zp, sizeof(zp), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(b->d_tab->dem_ntab + slot, &np, sizeof(np), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  b->book.set_slot(kSceneDem, slot, dem_geom(c));
  return MPPI_OK;
}

int mppi_batch_set_costmap(mppi_batch* b, int32_t slot, const float* cm_host) {
  if (int rc = slot_index(b, kSceneCostmap, slot)) return rc;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  if (!cm_host) return slot_free(b, kSceneCostmap, slot);
  DeviceBuf<float> fresh;
  float* dst = nullptr;
  if (int rc = costmap_slot_buffer(b, slot, "batch_set_costmap", fresh, &dst)) return rc;
  HIP_TRY(hipMemcpyAsync(dst, cm_host, (size_t)c->cmap.size * c->cmap.size * sizeof(float), hipMemcpyHostToDevice,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return costmap_slot_publish(b, slot, fresh);
}

int mppi_batch_build_costmap(mppi_batch* b, int32_t slot, const double* obstacles, int32_t n, double origin_x,
                             double origin_y, double r_robot, int32_t power, int32_t metric, float* out_host) {
  return mppi_batch_build_costmap_hazard(b, slot, -1, obstacles, n, origin_x, origin_y, r_robot, power, metric, nullptr,
                                         out_host, nullptr);
}

int mppi_batch_build_costmap_hazard(mppi_batch* b, int32_t slot, int32_t dem_slot, const double* obstacles, int32_t n,
                                    double origin_x, double origin_y, double r_robot, int32_t power, int32_t metric,
                                    const mppi_hazard* hz, float* out_host, uint8_t* mask_host) {
  if (int rc = slot_index(b, kSceneCostmap, slot)) return rc;
  mppi_ctx* c = b->c;
  // the heights a hazard build reads: a DEM slot of the batch, or the context's DEM
  DemView dem;
  if (hz) {
    if (dem_slot != -1) {
      if (int rc = slot_index(b, kSceneDem, dem_slot)) return rc;
      if (!b->dems[dem_slot].Z)
        return fail(MPPI_ESTATE, "batch_build_costmap_hazard: dem_slot " + std::to_string(dem_slot) + " is empty");
      dem = dem_view(b->dems[dem_slot]);
    } else {
      if (!c->dem.Z || c->dem.rows <= 0)
        return fail(MPPI_ESTATE, "batch_build_costmap_hazard: no DEM bound: call mppi_set_dem first");
      dem = dem_view(c->dem);
    }
  }
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  // the builder's own resolution (mppi_build_costmap) must be the one the kernels index the slots with
  const double hw = (double)c->cmap.hw;
  if (c->cmap.size > 0 && (float)(2 * hw / c->cmap.size) != c->cmap.res)
    return fail(MPPI_EINVAL, "batch_build_costmap: the context costmap's resolution is not 2 * half_width / size");
  DeviceBuf<float> fresh;
  float* dst = nullptr;
  if (int rc = costmap_slot_buffer(b, slot, "batch_build_costmap", fresh, &dst)) return rc;
  if (int rc = build_costmap_into(c, obstacles, n, c->cmap.size, hw, origin_x, origin_y, r_robot, power, metric, dst,
                                  out_host, hz, &dem, mask_host))
    return rc;
  return costmap_slot_publish(b, slot, fresh);
}

int mppi_batch_set_episode_scene(mppi_batch* b, int32_t e, int32_t dem_slot, int32_t costmap_slot) {
  if (int rc = batch_episode(b, e)) return rc;
  if (int rc = campaign_busy(b, "batch_set_episode_scene")) return rc;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  SceneKind bad = kSceneDem;
  const SceneRecord before = b->book.record(e);
  const SceneError err = b->book.set_episode_scene(e, dem_slot, costmap_slot, &bad);
  if (err != kSceneOk) {
    const int32_t s = bad == kSceneDem ? dem_slot : costmap_slot;
    const std::string what = std::string(bad == kSceneDem ? "DEM" : "costmap") + " slot " + std::to_string(s);
    if (err == kSceneSlotRange)
      return fail(MPPI_EINVAL, "episode " + std::to_string(e) + ": " + what + " outside [-1, " +
                                   std::to_string(b->book.slots(bad)) + ")");
    return fail(MPPI_EINVAL, "episode " + std::to_string(e) + ": " + what + " is empty");
  }
  HIP_TRY(hipSetDevice(c->device));
  return push_scene(b, e, before);
}

int mppi_batch_set_episode_trajectories(mppi_batch* b, int32_t e, int64_t num_trajectories) {
  if (int rc = batch_episode(b, e)) return rc;
  if (int rc = campaign_busy(b, "batch_set_episode_trajectories")) return rc;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  const SceneRecord before = b->book.record(e);
  if (b->book.set_episode_K(e, num_trajectories) != kSceneOk)
    return fail(MPPI_EINVAL, "episode " + std::to_string(e) + ": num_trajectories " + std::to_string(num_trajectories) +
                                 " outside [1, " + std::to_string(c->p.num_trajectories) + "] (0: the context's)");
  HIP_TRY(hipSetDevice(c->device));
  return push_scene(b, e, before);
}

static int slope_mode_check(int32_t slope_mode, const char* who) {
  if (slope_mode == MPPI_SLOPE_BODY || slope_mode == MPPI_SLOPE_WHEELS) return MPPI_OK;
  return fail(MPPI_EINVAL, std::string(who) + ": slope_mode must be MPPI_SLOPE_WHEELS or MPPI_SLOPE_BODY");
}

// mppi_batch_score and mppi_batch_score_ex: the slope term in its body form, or (wheels) over the wheel
// log's two contact paths; metrics [E] or null.
static int batch_score(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins, bool wheels,
                       mppi_path_scores* out, int32_t* rows, mppi_path_metrics* metrics) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (!out) return fail(MPPI_EINVAL, "null argument");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "batch_score: no costmap: call mppi_set_costmap first");
  if (wheels && !b->wbook.can_score_wheels((bool)b->log))
    return fail(MPPI_ESTATE, "batch_score: MPPI_SLOPE_WHEELS needs the wheel log: call mppi_batch_set_wheel_log(b, 1) "
                             "before the run (a log row alone has no wheel contacts)");
  if (int rc_g = scene_geometry(b)) return rc_g;
  HIP_TRY(hipSetDevice(c->device));
  const size_t E = (size_t)b->E;
  if (!b->log) {  // no run yet: no episode has a row
    if (metrics) std::memset(metrics, 0, E * sizeof(mppi_path_metrics));
    if (out->cost) std::memset(out->cost, 0, E * 4);
    if (out->terms) std::memset(out->terms, 0, E * 16);
    if (out->collisions) std::memset(out->collisions, 0, E * 4);
    if (rows) std::memset(rows, 0, E * 4);
    return MPPI_OK;
  }
  const mppi_params& p = c->p;
  // a tracked run began on the device: its start and goal are in the episode's tracking record
  std::vector<BatchTrackRec> trk;
  if (!origins && b->tracking && b->trk.keep_log) {
    trk.resize(E);
    HIP_TRY(hipMemcpyAsync(trk.data(), b->d_track, E * sizeof(BatchTrackRec), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  std::vector<ScoreGoal> goals(E);
  for (size_t e = 0; e < E; ++e) {
    mppi_state st{};
    if (origins) {
      st.x = origins[e].x;
      st.y = origins[e].y;
      st.goal_x = origins[e].goal_x;
      st.goal_y = origins[e].goal_y;
    } else if (!trk.empty()) {
      st.x = trk[e].acc.x0;
      st.y = trk[e].acc.y0;
      st.goal_x = trk[e].gx;
      st.goal_y = trk[e].gy;
    } else {
      st.x = b->origin[e][0];
      st.y = b->origin[e][1];
      st.goal_x = b->origin[e][2];
      st.goal_y = b->origin[e][3];
    }
    ServerCmd d;
    state_fields(p, st, d);
    goals[e] = ScoreGoal{d.gx, d.gy, d.igx, d.igy, d.pf_scale, d.pf_far, d.speed_on, d.x0, d.y0, 0};
  }
  // each path on its episode's costmap: the slot's where the episode holds one, else the context's
  // (no array at all while no episode in use holds a costmap slot)
  std::vector<const float*> cmaps;
  if (b->book.any_costmap_held()) {
    cmaps.resize(E);
    for (size_t e = 0; e < E; ++e) {
      const int s = b->book.costmap_of((int)e);
      cmaps[e] = s >= 0 ? b->cms[s].get() : c->cmap.cm.get();
    }
  }
  return score_logs(b, goals, cmaps, {}, b->log, &b->ep->steps_run, (int)(sizeof(BatchEpisode) / sizeof(int32_t)),
                    b->log_cap, yardstick, out, rows, "batch_score", wheels ? b->wlog.get() : nullptr, metrics);
}

int mppi_batch_score(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                     mppi_path_scores* out, int32_t* rows) {
  return batch_score(b, yardstick, origins, false, out, rows, nullptr);
}

int mppi_batch_score_ex(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                        int32_t slope_mode, mppi_path_scores* out, int32_t* rows, mppi_path_metrics* metrics) {
  if (int rc = slope_mode_check(slope_mode, "batch_score_ex")) return rc;
  return batch_score(b, yardstick, origins, slope_mode == MPPI_SLOPE_WHEELS, out, rows, metrics);
}

int mppi_batch_set_wheel_log(mppi_batch* b, int32_t enable) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  switch (b->wbook.set_wheel_log(enable != 0, b->campaign == mppi_batch::kUnfinished, b->tracking)) {
    case kWheelCampaign: return campaign_busy(b, "batch_set_wheel_log");
    case kWheelTracking: return tracking_busy(b, "batch_set_wheel_log");
    default: return MPPI_OK;
  }
}

int mppi_batch_set_score_options(mppi_batch* b, int32_t slope_mode, int32_t metrics) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  switch (b->wbook.set_score_options(slope_mode, metrics != 0, b->campaign == mppi_batch::kUnfinished, b->tracking)) {
    case kWheelSlopeMode: return slope_mode_check(slope_mode, "batch_set_score_options");
    case kWheelCampaign: return campaign_busy(b, "batch_set_score_options");
    case kWheelTracking: return tracking_busy(b, "batch_set_score_options");
    default: return MPPI_OK;
  }
}

int mppi_batch_get_wheel_log(mppi_batch* b, int32_t e, int32_t first, int32_t count, float* rows6) {
  if (int rc = batch_episode(b, e)) return rc;
  if (first < 0 || count < 0) return fail(MPPI_EINVAL, "wheel log range out of bounds");
  if (count > 0 && !rows6) return fail(MPPI_EINVAL, "null argument");
  if (!b->wbook.log_wheels())
    return fail(MPPI_ESTATE, "batch_get_wheel_log: the log has no wheel log beside it: call mppi_batch_set_wheel_log(b, 1) "
                             "before the run or before tracking is set");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  BatchEpisode& r = b->host[e];
  hipError_t he = hipMemcpyAsync(&r, b->ep + e, sizeof(BatchEpisode), hipMemcpyDeviceToHost, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he != hipSuccess) return after_wait(b, fail(MPPI_EHIP, std::string("batch_get_wheel_log: ") + hipGetErrorString(he)));
  if ((int64_t)first + count > r.steps_run)
    return after_wait(b, fail(MPPI_EINVAL, "wheel log range beyond the steps of the last run"));
  if (count > 0) {
    he = hipMemcpyAsync(rows6, b->wlog + ((size_t)e * b->log_cap + first) * 6, (size_t)count * 6 * sizeof(float),
                        hipMemcpyDeviceToHost, c->stream);
    if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
    if (he != hipSuccess) return after_wait(b, fail(MPPI_EHIP, std::string("batch_get_wheel_log: ") + hipGetErrorString(he)));
  }
  return after_wait(b, MPPI_OK);
}

int mppi_batch_get_run_metrics(mppi_batch* b, int32_t e, int32_t first, int32_t count, mppi_path_metrics* metrics) {
  if (int rc = batch_episode(b, e)) return rc;
  if (!b->tracking || !b->wbook.tracking().metrics)
    return fail(MPPI_ESTATE, "batch_get_run_metrics: tracking was not set with the metrics on: call "
                             "mppi_batch_set_score_options(b, slope_mode, 1), then mppi_batch_set_tracking");
  const int R = b->trk.runs_per_episode;
  if (first < 0 || count < 0 || (int64_t)first + count > R)
    return fail(MPPI_EINVAL, "batch_get_run_metrics: runs [" + std::to_string(first) + ", " +
                                 std::to_string((int64_t)first + count) + ") outside the " + std::to_string(R) +
                                 " result rows of an episode");
  if (count == 0) return MPPI_OK;
  if (!metrics) return fail(MPPI_EINVAL, "null argument");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  hipError_t he = hipMemcpyAsync(metrics, b->d_runmetrics + ((size_t)e * R + first), (size_t)count * sizeof(PathMetrics),
                                 hipMemcpyDeviceToHost, c->stream);
  if (he == hipSuccess) he = hipStreamSynchronize(c->stream);
  if (he != hipSuccess) return after_wait(b, fail(MPPI_EHIP, std::string("batch_get_run_metrics: ") + hipGetErrorString(he)));
  return after_wait(b, MPPI_OK);
}

// mppi_batch_set_tasks and mppi_batch_set_tasks_scored: one list, one set of checks.  scored: the
// lanes score as they run, with `yardstick` (NULL: the context's params); keep_log false (scored
// lists only): no arena.
static int set_tasks(mppi_batch* b, int32_t n, const mppi_batch_task* tasks, bool scored,
                     const mppi_batch_variant* yardstick, bool keep_log) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (n < 0) return fail(MPPI_EINVAL, "tasks: n must be >= 0");
  if (n > 0 && !tasks) return fail(MPPI_EINVAL, "null argument");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (int rc = tracking_busy(b, "batch_set_tasks")) return rc;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<TaskSpec> specs((size_t)n);
  for (int i = 0; i < n; ++i) {
    specs[i].variant = tasks[i].variant;
    specs[i].dem = tasks[i].dem_slot;
    specs[i].cm = tasks[i].costmap_slot;
    specs[i].K = tasks[i].num_trajectories;
    specs[i].max_steps = tasks[i].max_steps;
  }
  BatchTaskBook fresh;
  int bad = -1;
  SceneKind kind = kSceneDem;
  const TaskError err = fresh.set(specs, (int)b->variants.size(), b->book, dem_geom(c), costmap_geom(c),
                                  c->p.num_trajectories, &bad, &kind, keep_log);
  if (err != kTaskOk) return fail(MPPI_EINVAL, task_error(b, bad, tasks[bad], err, kind));
  // the list is replaced from here on: an unfinished campaign of the old one is abandoned
  if (b->campaign == mppi_batch::kUnfinished)
    if (int rc = campaign_restore(b)) return rc;
  task_list_clear(b);
  if (n == 0) return MPPI_OK;
  const size_t N = (size_t)n, E = (size_t)b->E;
  // the arena, and max_cap rows behind it: the scorer stages every path of a tile up to the tile's
  // longest, so it reads (and drops) up to that many rows past a short last task
  // (a list that keeps no log has no arena, and gives an earlier list's back: no kernel is in flight)
  const size_t log_bytes = keep_log ? ((size_t)fresh.total_rows() + (size_t)fresh.max_cap()) * 8 * sizeof(float) : 0;
  if (!keep_log) b->tlog.reset();
  // the options as they stand (mppi_batch_set_wheel_log / _set_score_options): tables only for those on
  // (task_list_clear dropped the old list's tables)
  BatchWheelBook wb = b->wbook;  // (the book takes the list once the tables stand)
  const WheelTables lt = wb.take_list(scored, keep_log);
  const bool wheels_log = lt.wlog, slope_wheels = lt.wacc, metrics = lt.metrics;
  if (b->d_tasks.grow(N * sizeof(BatchTask)) || b->d_res.grow(N * sizeof(BatchTaskResult)) ||
      b->d_lane.grow(E * sizeof(BatchLane)) || b->d_count.grow((E + 1) * sizeof(int)) ||
      (keep_log && b->tlog.grow(log_bytes)) || (wheels_log && b->twlog.grow(log_bytes / 8 * 6)) ||
      (slope_wheels && b->d_wacc.grow(E * sizeof(BatchWheelAcc))) ||
      (metrics && (b->d_macc.grow(E * sizeof(PathMetricsAcc)) || b->d_metrics.grow(N * sizeof(PathMetrics)))) ||
      (scored && (b->d_acc.grow(E * sizeof(BatchScoreAcc)) || b->d_score.grow(N * sizeof(BatchTaskScore))))) {
    (void)hipGetLastError();
    return fail(MPPI_EHIP, "tasks: allocation of the tables of " + std::to_string(n) + " tasks and a log arena of " +
                               std::to_string(log_bytes) + " bytes failed");
  }
  std::vector<BatchTask> dev(N);
  for (int i = 0; i < n; ++i) {
    ServerCmd d;
    state_fields(c->p, tasks[i].start, d);
    BatchTask& t = dev[i];
    t = BatchTask{};
    t.x0 = d.x0;
    t.y0 = d.y0;
    t.h0x = d.h0x;
    t.h0y = d.h0y;
    t.h0z = d.h0z;
    t.wl = d.wl;
    t.wr = d.wr;
    t.gx = d.gx;
    t.gy = d.gy;
    t.s1 = d.s1;
    t.s2 = d.s2;
    t.variant = tasks[i].variant;
    t.seed = tasks[i].seed;
    const SceneRecord r = fresh.record(i);
    t.scene = BatchScene{r.dem, r.cm, r.K, r.blocks};
    t.max_steps = tasks[i].max_steps;
    t.log_base = fresh.base(i);
  }
  HIP_TRY(hipMemcpyAsync(b->d_tasks, dev.data(), N * sizeof(BatchTask), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(b->d_res, 0, N * sizeof(BatchTaskResult), c->stream));
  if (scored) HIP_TRY(hipMemsetAsync(b->d_score, 0, N * sizeof(BatchTaskScore), c->stream));
  if (metrics) HIP_TRY(hipMemsetAsync(b->d_metrics, 0, N * sizeof(PathMetrics), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // dev is pageable and dies here
  b->tbook = fresh;
  b->tasks.assign(tasks, tasks + n);
  b->res.assign(N, BatchTaskResult{});
  b->scored = scored;
  b->wbook = wb;
  // the yardstick is taken here (as score_logs takes it when it scores a log)
  if (scored) b->yard = resolve_yardstick(c, yardstick);
  return MPPI_OK;
}

int mppi_batch_set_tasks(mppi_batch* b, int32_t n, const mppi_batch_task* tasks) {
  return set_tasks(b, n, tasks, false, nullptr, true);
}

int mppi_batch_set_tasks_scored(mppi_batch* b, int32_t n, const mppi_batch_task* tasks,
                                const mppi_batch_variant* yardstick, int32_t keep_log) {
  return set_tasks(b, n, tasks, true, yardstick, keep_log != 0);
}

int mppi_batch_get_task_scores(mppi_batch* b, int32_t first, int32_t count, mppi_path_scores* out, int32_t* rows,
                               double* length) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (b->tbook.empty() || !b->scored)
    return fail(MPPI_ESTATE, "batch_get_task_scores: the task list was not set scored: call mppi_batch_set_tasks_scored");
  if (first < 0 || count < 0 || (int64_t)first + count > b->tbook.size())
    return fail(MPPI_EINVAL, "batch_get_task_scores: tasks [" + std::to_string(first) + ", " +
                                 std::to_string((int64_t)first + count) + ") outside the list of " +
                                 std::to_string(b->tbook.size()) + " tasks");
  if (count == 0) return MPPI_OK;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  std::vector<BatchTaskScore> sc((size_t)count);
  HIP_TRY(hipMemcpyAsync(sc.data(), b->d_score + first, (size_t)count * sizeof(BatchTaskScore), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  for (int32_t i = 0; i < count; ++i) {
    const BatchTaskScore& r = sc[(size_t)i];
    if (out && out->cost) out->cost[i] = r.cost;
    if (out && out->terms) std::memcpy(out->terms + 4 * (size_t)i, r.terms, sizeof(r.terms));
    if (out && out->collisions) out->collisions[i] = r.collisions;
    if (rows) rows[i] = r.rows;
    if (length) length[i] = r.length;
  }
  return MPPI_OK;
}

int mppi_batch_run_tasks(mppi_batch* b, int32_t proj, int32_t n_steps, const mppi_loop_policy* policy,
                         int32_t* tasks_done, int64_t* batch_steps) {
  if (!b || !policy) return fail(MPPI_EINVAL, "null argument");
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  if (n_steps < 0) return fail(MPPI_EINVAL, "n_steps must be >= 0");
  if (policy->check_every < 0) return fail(MPPI_EINVAL, "check_every must be >= 0");
  if (!(policy->sigma_div != 0.0f)) return fail(MPPI_EINVAL, "sigma_div must be non-zero");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (b->tbook.empty()) return fail(MPPI_ESTATE, "batch_run_tasks: no task list: call mppi_batch_set_tasks first");
  if (int rc = tracking_busy(b, "batch_run_tasks")) return rc;
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM: call mppi_set_dem first");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "no costmap: call mppi_set_costmap first");
  int s = b->tbook.mismatch(kSceneDem, b->book, dem_geom(c));
  if (s >= 0)
    return fail(MPPI_ESTATE, "batch_run_tasks: DEM slot " + std::to_string(s) +
                                 " was set with another geometry than the context's current DEM");
  s = b->tbook.mismatch(kSceneCostmap, b->book, costmap_geom(c));
  if (s >= 0)
    return fail(MPPI_ESTATE, "batch_run_tasks: costmap slot " + std::to_string(s) +
                                 " was set with another geometry than the context's current costmap");
  HIP_TRY(hipSetDevice(c->device));
  const int rc = campaign_run(b, proj, n_steps, *policy, tasks_done, batch_steps);
  if (rc == MPPI_EHIP) b->failed = true;
  return rc;
}

static int batch_task(mppi_batch* b, int32_t i) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (i < 0 || i >= b->tbook.size())
    return fail(MPPI_EINVAL, "task index " + std::to_string(i) + " outside the list of " +
                                 std::to_string(b->tbook.size()) + " tasks");
  return MPPI_OK;
}

int mppi_batch_get_task(mppi_batch* b, int32_t i, mppi_state* state, int32_t* steps, int32_t* reached,
                        int32_t* started) {
  if (int rc = batch_task(b, i)) return rc;
  const BatchTaskResult& r = b->res[i];  // the host's copy: mppi_batch_run_tasks read it back
  if (state) {
    if (r.flags == 0) {
      *state = b->tasks[i].start;
    } else {
      state->x = r.x0;
      state->y = r.y0;
      state->heading[0] = r.h0x;
      state->heading[1] = r.h0y;
      state->heading[2] = r.h0z;
      state->left_wheel_speed = r.wl;
      state->right_wheel_speed = r.wr;
      state->goal_x = r.gx;
      state->goal_y = r.gy;
      state->std_dev_u1 = r.s1;
      state->std_dev_u2 = r.s2;
    }
  }
  if (steps) *steps = r.steps;
  if (reached) *reached = r.reached;
  if (started) *started = (r.flags & 2) ? 2 : (r.flags & 1);
  return MPPI_OK;
}

int mppi_batch_get_task_log(mppi_batch* b, int32_t i, int32_t first, int32_t count, float* rows) {
  if (int rc = batch_task(b, i)) return rc;
  if (first < 0 || count < 0) return fail(MPPI_EINVAL, "log range out of bounds");
  if (count > 0 && !rows) return fail(MPPI_EINVAL, "null argument");
  if ((int64_t)first + count > b->res[i].steps)
    return fail(MPPI_EINVAL, "task " + std::to_string(i) + ": log range beyond the " + std::to_string(b->res[i].steps) +
                                 " steps the task has taken");
  if (!b->tbook.keeps_log()) return fail(MPPI_ESTATE, "batch_get_task_log: the task list keeps no log (keep_log = 0)");
  if (count == 0) return MPPI_OK;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(rows, b->tlog + ((size_t)b->tbook.base(i) + first) * 8, (size_t)count * 8 * sizeof(float),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_batch_get_task_wheel_log(mppi_batch* b, int32_t i, int32_t first, int32_t count, float* rows6) {
  if (int rc = batch_task(b, i)) return rc;
  if (first < 0 || count < 0) return fail(MPPI_EINVAL, "wheel log range out of bounds");
  if (count > 0 && !rows6) return fail(MPPI_EINVAL, "null argument");
  if ((int64_t)first + count > b->res[i].steps)
    return fail(MPPI_EINVAL, "task " + std::to_string(i) + ": wheel log range beyond the " +
                                 std::to_string(b->res[i].steps) + " steps the task has taken");
  if (!b->wbook.list().wlog)
    return fail(MPPI_ESTATE, "batch_get_task_wheel_log: the task list keeps no wheel log: call "
                             "mppi_batch_set_wheel_log(b, 1) before the list is set (and keep its log)");
  if (count == 0) return MPPI_OK;
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(rows6, b->twlog + ((size_t)b->tbook.base(i) + first) * 6, (size_t)count * 6 * sizeof(float),
                         hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_batch_get_task_metrics(mppi_batch* b, int32_t first, int32_t count, mppi_path_metrics* metrics) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (b->tbook.empty() || !b->scored || !b->wbook.list().metrics)
    return fail(MPPI_ESTATE, "batch_get_task_metrics: the task list was not set scored with the metrics on: call "
                             "mppi_batch_set_score_options(b, slope_mode, 1), then mppi_batch_set_tasks_scored");
  if (first < 0 || count < 0 || (int64_t)first + count > b->tbook.size())
    return fail(MPPI_EINVAL, "batch_get_task_metrics: tasks [" + std::to_string(first) + ", " +
                                 std::to_string((int64_t)first + count) + ") outside the list of " +
                                 std::to_string(b->tbook.size()) + " tasks");
  if (count == 0) return MPPI_OK;
  if (!metrics) return fail(MPPI_EINVAL, "null argument");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(metrics, b->d_metrics + first, (size_t)count * sizeof(PathMetrics), hipMemcpyDeviceToHost,
                         c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

static int batch_score_tasks(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins, bool wheels,
                             mppi_path_scores* out, int32_t* rows, mppi_path_metrics* metrics) {
  if (!b) return fail(MPPI_EINVAL, "null batch");
  if (!out) return fail(MPPI_EINVAL, "null argument");
  mppi_ctx* c = b->c;
  if (int rc_q = quiesce(c)) return rc_q;
  if (b->failed) return fail(MPPI_ESTATE, "batch: a HIP error ended an earlier run");
  if (b->tbook.empty()) return fail(MPPI_ESTATE, "batch_score_tasks: no task list: call mppi_batch_set_tasks first");
  if (!b->tbook.keeps_log()) return fail(MPPI_ESTATE, "batch_score_tasks: the task list keeps no log (keep_log = 0)");
  if (wheels && !b->wbook.list().wlog)
    return fail(MPPI_ESTATE, "batch_score_tasks: MPPI_SLOPE_WHEELS needs the wheel log: call "
                             "mppi_batch_set_wheel_log(b, 1) before the list is set (a log row alone has no wheel contacts)");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "batch_score_tasks: no costmap: call mppi_set_costmap first");
  const int s = b->tbook.mismatch(kSceneCostmap, b->book, costmap_geom(c));
  if (s >= 0)
    return fail(MPPI_ESTATE, "batch_score_tasks: costmap slot " + std::to_string(s) +
                                 " was set with another geometry than the context's current costmap");
  HIP_TRY(hipSetDevice(c->device));
  const size_t N = (size_t)b->tbook.size();
  std::vector<ScoreGoal> goals(N);
  std::vector<int64_t> base(N);
  for (size_t i = 0; i < N; ++i) {
    const mppi_state& o = origins ? origins[i] : b->tasks[i].start;
    mppi_state st{};
    st.x = o.x;
    st.y = o.y;
    st.goal_x = o.goal_x;
    st.goal_y = o.goal_y;
    ServerCmd d;
    state_fields(c->p, st, d);
    goals[i] = ScoreGoal{d.gx, d.gy, d.igx, d.igy, d.pf_scale, d.pf_far, d.speed_on, d.x0, d.y0, 0};
    base[i] = b->tbook.base((int)i);
  }
  // each path on its task's costmap (no array at all while no listed task holds a costmap slot)
  std::vector<const float*> cmaps;
  if (b->tbook.any_costmap()) {
    cmaps.resize(N);
    for (size_t i = 0; i < N; ++i) {
      const int cs = b->tbook.task((int)i).cm;
      cmaps[i] = cs >= 0 ? b->cms[cs].get() : c->cmap.cm.get();
    }
  }
  // lengths: the result table's own step counts (0 for a task that has not ended)
  return score_logs(b, goals, cmaps, base, b->tlog, &b->d_res->steps, (int)(sizeof(BatchTaskResult) / sizeof(int32_t)),
                    b->tbook.max_cap(), yardstick, out, rows, "batch_score_tasks", wheels ? b->twlog.get() : nullptr,
                    metrics);
}

int mppi_batch_score_tasks(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                           mppi_path_scores* out, int32_t* rows) {
  return batch_score_tasks(b, yardstick, origins, false, out, rows, nullptr);
}

int mppi_batch_score_tasks_ex(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                              int32_t slope_mode, mppi_path_scores* out, int32_t* rows, mppi_path_metrics* metrics) {
  if (int rc = slope_mode_check(slope_mode, "batch_score_tasks_ex")) return rc;
  return batch_score_tasks(b, yardstick, origins, slope_mode == MPPI_SLOPE_WHEELS, out, rows, metrics);
}

}  // extern "C"
