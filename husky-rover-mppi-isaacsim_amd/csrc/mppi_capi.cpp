// C-ABI implementation (include/mppi.h): context, buffers, launch planning, host<->device copies.
//
// Host arithmetic that feeds the kernels (path-follow branch, intermediate
// goal, window bounds) is float32 in the reference's operation order; this
// file is compiled with -ffp-contract=off like the kernels.
//
// The other subsystems of the C-ABI are in mppi_capi_costmap.cpp, mppi_capi_score.cpp,
// mppi_capi_bilinear.cpp, mppi_capi_group.cpp and mppi_capi_batch.cpp; mppi_ctx.h is what they share.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "mppi.h"
#include "mppi_ctx.h"
#include "mppi_kernels.h"
#include "mppi_python25d.h"

using namespace mppi;
using namespace mppi::capi;

namespace mppi {
namespace capi {

thread_local std::string g_err;

int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// Reciprocal y for cdiv_f(a, b, y) that reproduces the IEEE quotient for every
// significand (checked exhaustively on the device, 2^23 cases); 0 if none of
// RN(1/b) and its two neighbours qualifies.  Cached per divisor.
int verified_reciprocal(mppi_ctx* c, float b, float* y_out) {
  if (!c->use_cdiv) {  // mppi_set_option "verified_reciprocal" 0
    *y_out = 0.0f;
    return MPPI_OK;
  }
  uint32_t key;
  std::memcpy(&key, &b, 4);
  auto it = c->cdiv_cache.find(key);
  if (it != c->cdiv_cache.end()) {
    *y_out = it->second;
    return MPPI_OK;
  }
  float y = 0.0f;
  if (std::isfinite(b) && b != 0.0f) {
    const float y0 = (float)(1.0 / (double)b);
    const float cand[3] = {y0, std::nextafter(y0, 0.0f), std::nextafter(y0, 2.0f * y0)};
    for (float yc : cand) {
      unsigned bad = 1;
      HIP_TRY(hipMemsetAsync(c->cdiv_bad, 0, sizeof(unsigned), c->stream));
      HIP_TRY(launch_cdiv_verify(b, yc, c->cdiv_bad, c->stream));
      HIP_TRY(hipMemcpyAsync(&bad, c->cdiv_bad, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));
      if (bad == 0) {
        y = yc;
        break;
      }
    }
  }
  c->cdiv_cache[key] = y;
  *y_out = y;
  return MPPI_OK;
}

static double now_us() {
  return std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

int check_ready(mppi_ctx* c) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (!c->dem.Z) return fail(MPPI_ESTATE, "no DEM: call mppi_set_dem first");
  if (!c->cmap.cm) return fail(MPPI_ESTATE, "no costmap: call mppi_set_costmap first");
  if (!c->sb.have_state) return fail(MPPI_ESTATE, "no state: call mppi_set_state first");
  HIP_TRY(hipSetDevice(c->device));
  return MPPI_OK;
}

// Launch geometry.  The rollouts of one step stay within H*dt*|v|max (+ wheel offset) of the robot:
// the square DEM window of that radius (every cell any lane can touch) is reported, not staged.
Plan make_plan(const mppi_ctx* c) {
  Plan pl;
  const int H = H_of(c);
  const double vabs = std::max(std::fabs((double)c->p.v_min_linear), std::fabs((double)c->p.v_max_linear));
  const double reach = (double)H * (double)c->p.dt * vabs + std::fabs((double)c->p.wheel_offset) * 1.01 + 0.01;
  const int Rc = (int)std::ceil(reach / (double)c->dem.res) + 3;
  const int64_t span = 2 * (int64_t)Rc + 2;
  pl.W = (int)std::min<int64_t>(span, c->dem.cols);
  pl.Wr = (int)std::min<int64_t>(span, c->dem.rows);
  const int64_t K = c->p.num_trajectories;
  // rollout kernel: chain + side waves per 64 trajectories, DEM and normals through L1/L2,
  // rings [D][PAIR_RING_IN + 4][TB] + cost[TB] + flags + nominal + leaf scratch in LDS (profiles/r01_notes.md)
  const int TB = PAIR_TRAJ;
  pl.traj_per_block = TB;
  pl.blocks = (int)((K + TB - 1) / TB);
  // role split where the rollout is latency-bound (at most one workgroup per CU); the pair
  // kernel's 8 waves per workgroup pack 4 workgroups per CU at larger K (MPPI_ROLES=0/1 forces)
  pl.roles = c->roles < 0 ? pl.blocks <= c->num_cus : c->roles != 0;
  pl.block = (pl.roles ? ROLES_WAVES_PER_TRAJ_WAVE : 2) * TB;
  const size_t scratch = ((size_t)(TB + TB / 64) * 4 + 15) / 16 * 16 + (size_t)(TB / 256) * (2 * H + 2) * sizeof(double);
  const size_t ring_rows = pl.roles ? (size_t)4 * PAIR_RING + 4 * ROLES_RING_OUT + 2 : (size_t)(PAIR_RING_IN + 4) * PAIR_RING + 1;
  pl.lds_bytes = ring_rows * TB * sizeof(float) + 4 * (TB / 64) * sizeof(int) +
                 (size_t)((2 * H + 3) & ~3) * sizeof(float) + scratch;
  // only at one workgroup per CU (the role-split kernel always: beyond one block per CU its
  // workgroups run the blocks in turn; the pair kernel up to one block per CU): the cache takes
  // the CU's spare LDS, which a co-resident pair workgroup (C5: 4 per CU) would need instead
  pl.grid = pl.roles ? std::min(pl.blocks, std::max(c->num_cus, 1)) : pl.blocks;
  if (pl.roles || pl.blocks <= c->num_cus) {
    // the rest of the CU's LDS keeps the sampled controls of the first steps ([2][T][TB]
    // floats, 16-byte aligned after the scratch), so the leaf reduction re-reads only the
    // other steps' normals from HBM (all workgroups reduce at once: a bandwidth burst)
    // room is left for the deferred optimal rollout of the previous step (mppi_tail_kernel,
    // 12H + 4 floats), which runs beside a rollout workgroup on one CU
    const size_t base = (pl.lds_bytes + 15) / 16 * 16;
    const size_t row2 = (size_t)2 * (TB + 4) * sizeof(float);  // UCACHE_ROW: one float4 of bank skew
    // (1 KiB more: the server kernel's static command / ticket words and LDS allocation granularity)
    const size_t budget = kLdsBytes - ((size_t)(12 * H + 4) * sizeof(float) + 2047) / 1024 * 1024 - 1024;
    pl.ucache_steps = base < budget ? (int)std::min<size_t>((size_t)H, (budget - base) / row2) : 0;
    if (pl.ucache_steps > 0) pl.lds_bytes = base + (size_t)pl.ucache_steps * row2;
  }
  // finish kernel: tree phase [16][2H+2] doubles + 64 x (15 PairScale + 16 m); phase 2
  // uo[2][PS] v[H] w[H] sin[H] cos[H] chain[12H] out[16H] lr[2][PS] floats (fin_phase2_floats)
  pl.fin_tree_bytes = (size_t)16 * (2 * H + 2) * sizeof(double) + (size_t)64 * (15 * 16 + 16 * 4);
  pl.fin_lds_bytes = std::max(pl.fin_tree_bytes, ((size_t)fin_phase2_floats(H) * sizeof(float) + 15) / 16 * 16);
  return pl;
}

// Noise grid: 4 four-wave workgroups per CU.  The noise of step i+2 runs beside the finish of
// step i and the start of rollout i+1 (4 per CU measured best at C3: 10095 steps/s against 9920 at
// 3 and 9730 at 2, alternating runs, profiles/r02_notes.md).
static int noise_groups(const mppi_ctx* c) { return std::max(c->num_cus, 1) * 4; }

static int ensure_nodes(mppi_ctx* c, int blocks) {
  const size_t need = (size_t)std::max(blocks, 1) * E_of(c);
  if (need <= c->sb.nodes_cap) return MPPI_OK;
  c->sb.nodes_cap = 0;
  HIP_TRY(c->sb.nodes.alloc(need * sizeof(double)));
  HIP_TRY(c->sb.rec_m.alloc((size_t)std::max(blocks, 1) * sizeof(float)));
  const size_t half = ((size_t)std::max(blocks, 1) + 1) / 2 * E_of(c);
  HIP_TRY(c->sb.scratch0.alloc(half * sizeof(double)));
  HIP_TRY(c->sb.scratch1.alloc(half * sizeof(double)));
  c->sb.nodes_cap = need;
  return MPPI_OK;
}

// The rollout / finish fields that follow from the robot state, in the server command's layout
// (fill_rollout copies them into the launch arguments).
void state_fields(const mppi_params& p, const mppi_state& st, ServerCmd& d) {
  d.x0 = st.x;
  d.y0 = st.y;
  d.h0x = st.heading[0];
  d.h0y = st.heading[1];
  d.h0z = st.heading[2];
  d.wl = st.left_wheel_speed;
  d.wr = st.right_wheel_speed;
  d.gx = st.goal_x;
  d.gy = st.goal_y;
  d.s1 = st.std_dev_u1;
  d.s2 = st.std_dev_u2;
  // _path_follow_critic / _maximise_speed scalar parts (critics_warp.py:111-123, :281-286)
  const float xd = st.goal_x - st.x;
  const float yd = st.goal_y - st.y;
  const float dist = std::sqrt(xd * xd + yd * yd);
  const float horizon = p.horizon;
  d.pf_far = dist > horizon ? 1 : 0;
  d.igx = st.x + (xd * horizon) / (dist + 1e-6f);
  d.igy = st.y + (yd * horizon) / (dist + 1e-6f);
  d.pf_scale = 1.0f + (2.0f * horizon) / dist;
  d.speed_on = (dist < 2.0f) ? 0 : 1;
}

std::string critics_error(const mppi_critics& k, int H) {
  if (k.slope_mode != MPPI_SLOPE_WHEELS && k.slope_mode != MPPI_SLOPE_BODY)
    return "slope_mode must be MPPI_SLOPE_WHEELS (0) or MPPI_SLOPE_BODY (1), got " + std::to_string(k.slope_mode);
  if (!std::isfinite(k.w_orientation)) return "w_orientation must be finite";
  if (k.w_orientation != 0.0f && H < 2)
    return "w_orientation != 0 needs num_iterations >= 2 (the rollout's last displacement)";
  return std::string();
}

std::string sampling_error(const mppi_sampling& s, int64_t k_offset) {
  if (s.antithetic != 0 && s.antithetic != 1) return "antithetic must be 0 or 1, got " + std::to_string(s.antithetic);
  if (s.nominal != 0 && s.nominal != 1) return "nominal must be 0 or 1, got " + std::to_string(s.nominal);
  if (!std::isfinite(s.beta) || !(s.beta >= 0.0f) || !(s.beta < 1.0f)) return "beta must be finite and in [0, 1)";
  if (s.antithetic && (k_offset & 1))
    return "antithetic needs an even k_offset (a pair is global k, k + 1), got " + std::to_string(k_offset);
  return std::string();
}

SamplePlan device_plan(const mppi_sampling& s) {
  SamplePlan r;
  r.antithetic = s.antithetic;
  r.nominal = s.nominal;
  r.beta = s.beta;
  r.g = (float)std::sqrt(1.0 - (double)s.beta * (double)s.beta);
  return r;
}

void fill_rollout(const mppi_ctx* c, const Plan& pl, const mppi_state& st, uint64_t step,
                  const float* unom, RolloutArgs& a) {
  const mppi_params& p = c->p;
  const int H = p.num_iterations;
  std::memset(&a, 0, sizeof(a));
  a.K = p.num_trajectories;
  a.ucache_steps = pl.ucache_steps;
  a.k_offset = p.k_offset;
  a.H = H;
  a.Z = c->dem.Z;
  a.ntab = c->dem.ntab;
  a.rows = c->dem.rows;
  a.grid = c->dem.cols;
  a.x_min = c->dem.x_min;
  a.y_min = c->dem.y_min;
  a.res = c->dem.res;
  a.cm = c->cmap.cm;
  a.cm_size = c->cmap.size;
  a.hw = c->cmap.hw;
  a.res_c = c->cmap.res;
  a.rinv_res = c->dem.rinv_res;
  a.cdiv_res = c->dem.rinv_res != 0.0f;
  a.rinv_res_c = c->cmap.rinv_res;
  a.cdiv_res_c = c->cmap.rinv_res != 0.0f;
  ServerCmd d;
  state_fields(p, st, d);
  a.x0 = d.x0;
  a.y0 = d.y0;
  a.h0x = d.h0x;
  a.h0y = d.h0y;
  a.h0z = d.h0z;
  a.wl = d.wl;
  a.wr = d.wr;
  a.gx = d.gx;
  a.gy = d.gy;
  a.s1 = d.s1;
  a.s2 = d.s2;
  a.pf_far = d.pf_far;
  a.igx = d.igx;
  a.igy = d.igy;
  a.pf_scale = d.pf_scale;
  a.speed_on = d.speed_on;
  a.seed = p.seed;
  a.n_base = step * (uint64_t)((H + 1) / 2);
  a.u_nom1 = unom;
  a.u_nom2 = unom + H;
  a.min_u1 = p.min_u1;
  a.max_u1 = p.max_u1;
  a.min_u2 = p.min_u2;
  a.max_u2 = p.max_u2;
  a.fk = p.filter_k;
  a.fa = p.filter_a;
  a.rwheel = p.robot_radius;
  a.vmin = p.v_min_linear;
  a.vmax = p.v_max_linear;
  a.wmin = p.v_min_angular;
  a.wmax = p.v_max_angular;
  a.dt = p.dt;
  a.off = p.wheel_offset;
  a.w_path = p.w_path;
  a.w_slope = p.w_slope;
  a.w_speed = p.w_speed;
  a.w_obs = p.w_obstacle;
  a.slope_body = c->crit.slope_mode == MPPI_SLOPE_BODY;
  a.w_orient = c->crit.w_orientation;
  a.thr = p.collision_threshold;
  a.pen = p.collision_penalty;
  a.T = p.temperature;
  a.cost_out = c->sb.cost;
  a.clk = c->sb.clk;
  a.nodes = c->sb.nodes;
  a.rec_m = c->sb.rec_m;
  a.ustore = c->sb.ustore;
  a.inj_u1 = c->sb.inj1;
  a.inj_u2 = c->sb.inj2;
  a.wave_prio = 1;
  // |w dt| < pi/4 for every clamped w: sin / cos without the range reduction (same bits)
  a.small_angle = std::max(std::fabs(p.v_min_angular), std::fabs(p.v_max_angular)) * p.dt < 0.78f;
}

void fill_finish(const mppi_ctx* c, const Plan& pl, const mppi_state& st, FinishArgs& f) {
  const mppi_params& p = c->p;
  std::memset(&f, 0, sizeof(f));
  f.H = p.num_iterations;
  f.T = p.temperature;
  f.scratch0 = c->sb.scratch0;
  f.scratch1 = c->sb.scratch1;
  f.uopt = c->sb.uopt;
  f.u_nom_next = c->sb.u_nom[c->sb.cur ^ 1];
  f.out = c->sb.stage;
  f.Z = c->dem.Z;
  f.ntab = c->dem.ntab;
  f.rows = c->dem.rows;
  f.grid = c->dem.cols;
  f.x_min = c->dem.x_min;
  f.y_min = c->dem.y_min;
  f.res = c->dem.res;
  f.rinv_res = c->dem.rinv_res;
  f.cdiv_res = c->dem.rinv_res != 0.0f;
  f.x0 = st.x;
  f.y0 = st.y;
  f.h0x = st.heading[0];
  f.h0y = st.heading[1];
  f.h0z = st.heading[2];
  f.wl = st.left_wheel_speed;
  f.wr = st.right_wheel_speed;
  f.ok = p.opt_filter_k;
  f.oa = p.opt_filter_a;
  f.rwheel = p.robot_radius;
  f.vmin = p.v_min_linear;
  f.vmax = p.v_max_linear;
  f.wmin = p.v_min_angular;
  f.wmax = p.v_max_angular;
  f.dt = p.dt;
  f.off = p.wheel_offset;
}

static void collect_timing(mppi_ctx* c) {
  float ms = 0.f;
  // mode 2: the host spun on the completion word, which the finish (enqueued after ev[1])
  // publishes, so ev[1] has retired already
  if (c->tm.roll_pending && hipEventSynchronize(c->tm.ev[1]) == hipSuccess &&
      hipEventElapsedTime(&ms, c->tm.ev[0], c->tm.ev[1]) == hipSuccess) {
    c->tm.t_roll += ms;
    c->tm.launches += 1;
  }
  if (c->tm.fin_pending && hipEventElapsedTime(&ms, c->tm.ev[2], c->tm.ev[3]) == hipSuccess) c->tm.t_fin += ms;
  c->tm.roll_pending = c->tm.fin_pending = false;
}

// Tail timing events live on the side stream: fold them in once the tail is done.
static void collect_tail_timing(mppi_ctx* c) {
  if (!c->tm.tail_pending) return;
  float ms = 0.f;
  if (hipEventSynchronize(c->tm.ev[5]) == hipSuccess && hipEventElapsedTime(&ms, c->tm.ev[4], c->tm.ev[5]) == hipSuccess) {
    c->tm.t_tail += ms;
    c->tm.tail_launches += 1;
  }
  c->tm.tail_pending = false;
}

static int enqueue_tail(mppi_ctx* c, const FinishArgs& f, int par);

// Launch the server's deferred tail of the last step (its completion word has been seen).
static int flush_tail(mppi_ctx* c) {
  if (!c->tail.pol.deferred) return MPPI_OK;
  c->tail.pol.deferred = false;
  return enqueue_tail(c, c->tail.def, c->tail.pol.def_slot);
}

// Drain every stream a tail may still run on, then wait for the tails' events.
int TailRing::drain() {
  // The tails' streams are drained, not only their events, the latest tail's last: a stream's first
  // synchronize after a kernel costs ~8-15 us of runtime work even when the kernel is long done
  // (profiles/ubench/devsync.hip), which the caller's next device synchronize would pay otherwise;
  // the older tails' stream is drained while the latest tail runs.
  hipStream_t last = pol.pending ? ts[pol.latest] : nullptr;
  for (int i = 0; i < kTailSlots; ++i)
    if (pol.inflight[i] && ts[i] && ts[i] != last) {
      const hipStream_t s = ts[i];
      HIP_TRY(hipStreamSynchronize(s));
      for (int j = 0; j < kTailSlots; ++j)
        if (ts[j] == s) pol.done(j);
    }
  if (last) HIP_TRY(hipStreamSynchronize(last));
  for (int i = 0; i < kTailSlots; ++i)
    if (pol.must_wait(i)) HIP_TRY(hipEventSynchronize(ev[i]));
  pol.all_done();
  return MPPI_OK;
}

// Wait until no deferred optimal rollout can still read tail_in or the DEM, and
// merge the latest one's outputs into out_host[4H, 16H).
static int sync_tail(mppi_ctx* c) {
  int rc = flush_tail(c);
  if (rc) return rc;
  if (!c->tail.pol.busy()) return MPPI_OK;
  rc = c->tail.drain();
  if (rc) return rc;
  collect_tail_timing(c);
  if (c->tail.pol.pending) {
    const int H = H_of(c);
    std::memcpy(c->sb.out_host.get() + 4 * H, c->tail.host[c->tail.pol.latest], (size_t)12 * H * sizeof(float));
    c->tail.pol.pending = false;
  }
  return MPPI_OK;
}

// Tell the running server to leave (it finishes the step it runs, reads its launch id in the command's stop slot
// and exits) without waiting: launches enqueued after it on the context stream run once it retired.
static void post_stop(mppi_ctx* c) {
  if (!c->srv.running) return;
  __atomic_store_n(&c->srv.cmd->slot[kCmdStopSlot], (uint64_t)c->srv.launch_id, __ATOMIC_RELEASE);
  c->srv.running = false;
  c->srv.exiting = true;
}

// Stop the resident server and wait until it has retired: every call on the context but mppi_step /
// set_state / get_outputs / get_timing starts with this.  Bounded (10 s: its workgroups must get CUs
// to leave, which another process's kernels can hold): MPPI_EHIP if it did not retire.
int quiesce(mppi_ctx* c) {
  if (!c) return MPPI_OK;
  post_stop(c);
  if (!c->srv.exiting) return MPPI_OK;
  hipSetDevice(c->device);
  const double t0 = now_us();
  for (;;) {
    const hipError_t e = hipStreamQuery(c->stream);
    if (e == hipSuccess) break;
    if (e != hipErrorNotReady) {
      c->srv.exiting = false;
      return fail(MPPI_EHIP, std::string("step server: ") + hipGetErrorString(e));
    }
    if (now_us() - t0 > 10e6) return fail(MPPI_EHIP, "the step server did not retire within 10 s of its stop");
    std::this_thread::yield();
  }
  c->srv.exiting = false;
  return MPPI_OK;
}

// Zero the finish handoff counter (level1_cnt[0]) and the server's record counter ([16]) after a
// step that did not complete them; no launch of the context may be running.
static void rearm_counters(mppi_ctx* c) {
  if (hipMemsetAsync(c->sb.level1_cnt, 0, 128, c->stream) == hipSuccess) hipStreamSynchronize(c->stream);
}

// Launch the resident server for the posted command `seq` (its first), with the plan of the last
// server_step (c->srv.pl ...).  Neither the relay nor the stop slot needs a reset: the relay's tags are
// older than this command, and the stop words hold an earlier launch's id, never this one's (a
// relaunch for the same command included).
static int launch_server(mppi_ctx* c, unsigned seq) {
  const Plan& pl = c->srv.pl;
  RolloutArgs a;
  fill_rollout(c, pl, c->sb.st, 0, c->sb.u_nom[c->sb.cur], a);  // (state, nominal buffer: from each command)
  ServerArgs z;
  std::memset(&z, 0, sizeof(z));
  fill_finish(c, pl, c->sb.st, z.f);
  z.f.recs = c->sb.nodes;
  z.f.rec_m = c->sb.rec_m;
  z.f.n_recs = pl.blocks;
  z.f.level1 = c->sb.level1;
  z.f.level1_cnt = c->sb.level1_cnt;
  z.f.abort = c->sb.level1_cnt + 24;  // (re-armed with the counters after a failed step)
  z.f.done = c->sb.done;
  z.nroll = pl.blocks;
  z.fin_P = c->srv.P;
  z.fin_ncol = c->srv.ncol;
  z.fin_groups = c->srv.groups;
  z.rec_cnt = c->sb.level1_cnt + 16;
  z.cmd = c->srv.cmd;
  z.relay = c->srv.relay;
  z.clk = c->sb.clk;
  for (int i = 0; i < kEpsSlots; ++i) z.eps[i] = c->ns.buf[i];
  z.u_nom[0] = c->sb.u_nom[0];
  z.u_nom[1] = c->sb.u_nom[1];
  for (int i = 0; i < kTailSlots; ++i) {
    z.tail_in[i] = c->tail.in[i];
    z.tail_out[i] = c->tail.host[i];
  }
  z.first_seq = seq;
  if (++c->srv.launch_id == 0) c->srv.launch_id = 1;
  z.launch_id = c->srv.launch_id;
  z.wait_ticks = c->srv.fin_wait_ticks;
  z.idle_ticks = c->srv.idle_us * 100;
  z.exit_after = c->srv.exit_after;
  z.plan = (unsigned)c->samp.antithetic | ((unsigned)c->samp.nominal << 1);  // (set_sampling stops the server)
  c->srv.exit_after = 0;  // (the hook applies to one launch)
  HIP_TRY(launch_step_server(a, z, c->srv.lds, c->stream, c->srv.proj));
  c->srv.running = true;
  ++c->srv.launches;
  return MPPI_OK;
}

// Spin until the finish has published c->sb.wait_seq (all outputs in pinned host memory).  A server
// that retired without taking the posted command (its head left on the idle limit just before the
// command was posted: an exit is all-or-nothing, so nothing of the step ran) is relaunched with the
// same command, counted in srv.relaunches; a fresh launch that retires without serving it fails the
// step.  A finish that gave up (done | kDoneFail), any other launch that retired without publishing,
// a stream error or 10 s without completion fail the step; the server is stopped and the counters
// re-armed.
static int wait_done(mppi_ctx* c) {
  if (c->tm.mode == 1) {  // the finish's timing events need the stream to retire
    HIP_TRY(hipStreamSynchronize(c->stream));
  }
  const unsigned want = c->sb.wait_seq;
  const double t0 = now_us();
  std::string why;
  c->srv.fail_kind = 0;
  bool relaunched = false;
  for (uint64_t i = 0;; ++i) {
    const unsigned v = __atomic_load_n(c->sb.done.get(), __ATOMIC_ACQUIRE);
    if (v == want) break;
    if (v == (want | kDoneFail)) {
      why = "the finish gave up waiting for the step's records";
      c->srv.fail_kind = 1;
      break;
    }
    if ((i & 255) == 255) {
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(c->sb.done.get(), __ATOMIC_ACQUIRE) == want) break;
        c->srv.running = false;  // (an idle server has exited: the stream is empty)
        if (c->srv.cmd_live && !relaunched) {
          relaunched = true;
          ++c->srv.relaunches;
          const int rc = launch_server(c, want);
          if (rc) {
            c->srv.cmd_live = false;
            return rc;
          }
          continue;
        }
        why = relaunched ? "a freshly launched step server retired without serving the step"
                         : "the step's launch retired without publishing its outputs";
        c->srv.fail_kind = 2;
        break;
      }
      if (e != hipErrorNotReady) {
        c->srv.cmd_live = false;
        return fail(MPPI_EHIP, std::string("step failed: ") + hipGetErrorString(e));
      }
      if (now_us() - t0 > 10e6) {
        why = "the step did not complete within 10 s";
        c->srv.fail_kind = 3;
        break;
      }
    }
    __builtin_ia32_pause();
  }
  if (c->srv.fail_kind == 0) {
    if (c->srv.cmd_live) c->srv.last_us = now_us();  // (the head polls for the next command from here)
    c->srv.cmd_live = false;
    return MPPI_OK;
  }
  c->srv.cmd_live = false;
  ++c->srv.failed;
  // (a server whose workgroups cannot all get CUs retires once they do: until then nothing may be
  // re-armed or rerun, and a server that never retires fails the call here)
  const std::string saved = why;
  if (quiesce(c)) {
    c->srv.fail_kind = 3;
    return fail(MPPI_EHIP, saved + "; " + g_err);
  }
  rearm_counters(c);
  // the normals the failed step's server was to generate may be incomplete: regenerate them
  if (c->last.resident && c->srv.cmd_noise >= 0) c->ns.pol.invalidate(c->srv.cmd_noise);
  return fail(MPPI_EHIP, why);
}

int NormalsSlots::ensure(size_t need, hipStream_t main) {
  if (need <= cap) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(main));
  HIP_TRY(hipStreamSynchronize(stream));
  pol.invalidate_all();
  cap = 0;
  for (auto& b : buf) b.reset();  // (all three before the first allocation: no more memory than the new slots need)
  for (auto& b : buf) HIP_TRY(b.alloc(need * sizeof(float)));
  cap = need;
  return MPPI_OK;
}

int NormalsSlots::settle_all(hipStream_t st, bool sync) {
  for (int i = 0; i < kEpsSlots; ++i)
    if (pol.pending[i]) {
      HIP_TRY(sync ? hipEventSynchronize(ev[i]) : hipStreamWaitEvent(st, ev[i], 0));
      pol.settled(i);
    }
  return MPPI_OK;
}

int NormalsSlots::settle(int slot, hipStream_t st, bool sync) {
  if (!pol.pending[slot]) return MPPI_OK;
  const hipError_t q = hipEventQuery(ev[slot]);
  if (q == hipErrorNotReady) HIP_TRY(sync ? hipEventSynchronize(ev[slot]) : hipStreamWaitEvent(st, ev[slot], 0));
  else if (q != hipSuccess) return fail(MPPI_EHIP, std::string("noise: ") + hipGetErrorString(q));
  pol.settled(slot);
  return MPPI_OK;
}

// Normals of Philox step `step` in an eps slot, generated on `st` if no slot holds them (first
// step, or a step counter that did not advance by one).  sync: wait for the slot on the host (the
// server reads it without stream order) instead of ordering `st` after it.
static int eps_for_step(mppi_ctx* c, const Plan& pl, uint64_t step, hipStream_t st, bool sync, int* slot_out) {
  NormalsSlots& ns = c->ns;
  int rc = ns.ensure((size_t)pl.blocks * 2 * H_of(c) * 256, c->stream);
  if (rc) return rc;
  const uint64_t nb = (uint64_t)((H_of(c) + 1) / 2);
  int slot = ns.pol.find(step);
  if (slot < 0) {
    // not precomputed: any in-flight fill must finish before a slot is reused
    rc = ns.settle_all(st, sync);
    if (rc) return rc;
    slot = 0;
    ns.pol.forget_steps();
    HIP_TRY(launch_noise(c->p.seed, step * nb, c->p.k_offset, pl.blocks, H_of(c), ns.buf[slot], st, noise_groups(c), device_plan(c->samp)));
    ns.pol.mark_ready(slot, step);
    if (sync) HIP_TRY(hipStreamSynchronize(st));
  } else {  // generated on the noise stream: before this rollout
    rc = ns.settle(slot, st, sync);
    if (rc) return rc;
  }
  *slot_out = slot;
  return MPPI_OK;
}

// After the rollout of `step` (which reads slot `used`) is enqueued: make sure the normals of steps
// step + 1 and step + 2 are generated or in flight, on the noise stream after the event `after` (recorded
// after this rollout, the last reader of a reused slot).  In steady state that is one launch, of step
// + 2's normals, which then has the finish, the host round trip and the whole next step to complete,
// so no rollout waits for it, and which runs beside the finish and the next rollout, not this one.
static int speculate_eps(mppi_ctx* c, const Plan& pl, uint64_t step, int used, hipEvent_t after) {
  const uint64_t nb = (uint64_t)((H_of(c) + 1) / 2);
  bool waited = false;
  for (int d = 1; d <= 2; ++d) {
    const uint64_t target = step + (uint64_t)d;
    if (c->ns.pol.holds(target)) continue;
    const int slot = c->ns.pol.victim(used, step);
    if (slot < 0) return fail(MPPI_ESTATE, "no free noise slot");
    if (!waited) {
      HIP_TRY(hipStreamWaitEvent(c->ns.stream, after, 0));
      waited = true;
    }
    HIP_TRY(launch_noise(c->p.seed, target * nb, c->p.k_offset, pl.blocks, H_of(c), c->ns.buf[slot], c->ns.stream,
                         noise_groups(c), device_plan(c->samp)));
    HIP_TRY(hipEventRecord(c->ns.ev[slot], c->ns.stream));
    c->ns.pol.mark_pending(slot, target);
  }
  return MPPI_OK;
}

// Run `launch` on `st` between the timing events ev[first] and ev[first + 1] when `timed`, and
// mark their pair pending for collect_timing / collect_tail_timing.
template <class Launch>
static int timed_launch(mppi_ctx* c, bool timed, int first, hipStream_t st, bool& pending, Launch launch) {
  if (timed) HIP_TRY(hipEventRecord(c->tm.ev[first], st));
  HIP_TRY(launch());
  if (timed) {
    HIP_TRY(hipEventRecord(c->tm.ev[first + 1], st));
    pending = true;
  }
  return MPPI_OK;
}

// Enqueue the rollout kernel for the current state / nominal sequence.
int enqueue_rollout(mppi_ctx* c, int proj, uint64_t step, int mode, const Plan& pl,
                    const float* unom, const mppi_state& st, const RolloutArgs* dump_args,
                    int* spec_slot) {
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  int rc = ensure_nodes(c, pl.blocks);
  if (rc) return rc;
  if (mode == 1) {  // injected controls: the leaf reads them back from here
    rc = grow(c->sb.ustore, (size_t)pl.blocks * pl.traj_per_block * 2 * H_of(c) * sizeof(float), c->stream);
    if (rc) return rc;
  }
  RolloutArgs a;
  fill_rollout(c, pl, st, step, unom, a);
  int eps_slot = -1;
  if (mode == 0 && pl.blocks > 0) {
    rc = eps_for_step(c, pl, step, c->stream, false, &eps_slot);
    if (rc) return rc;
    a.eps = c->ns.buf[eps_slot];
  }
  if (dump_args) {
    a.d_traj = dump_args->d_traj;
    a.d_hv = dump_args->d_hv;
    a.d_lw = dump_args->d_lw;
    a.d_rw = dump_args->d_rw;
    a.d_v = dump_args->d_v;
    a.d_w = dump_args->d_w;
    a.d_u1 = dump_args->d_u1;
    a.d_u2 = dump_args->d_u2;
  }
  if (pl.blocks == 0) return MPPI_OK;
  if (c->tm.mode && !dump_args) {
    // the rollout kernel's own time: nothing already enqueued on the side streams (the noise of a
    // later step, the previous step's deferred optimal rollout) runs beside the timed launch (both
    // modes, so that a kernel trace of the timing passes averages isolated launches only)
    HIP_TRY(hipEventRecord(c->tm.ev_side[0], c->ns.stream));
    HIP_TRY(hipEventRecord(c->tm.ev_side[1], c->tail.stream));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->tm.ev_side[0], 0));
    HIP_TRY(hipStreamWaitEvent(c->stream, c->tm.ev_side[1], 0));
  }
  rc = timed_launch(c, c->tm.mode && !dump_args, 0, c->stream, c->tm.roll_pending, [&] {
    return launch_rollout_pair(a, pl.grid, pl.lds_bytes, c->stream, proj, mode, dump_args != nullptr, pl.roles);
  });
  if (rc) return rc;
  if (eps_slot >= 0 && !dump_args && spec_slot && c->ns.late) {
    *spec_slot = eps_slot;  // (speculate_after: once the caller has enqueued the finish)
    return MPPI_OK;
  }
  if (eps_slot >= 0 && !dump_args) {  // the next steps' normals on the noise stream after this rollout
    HIP_TRY(hipEventRecord(c->ns.ev_prev_roll, c->stream));
    return speculate_eps(c, pl, step, eps_slot, c->ns.ev_prev_roll);
  }
  return MPPI_OK;
}

// The next steps' normals of a rollout enqueued with spec_slot set, ordered after what the context
// stream holds now (the finish): no event marker between the rollout and the finish.
static int speculate_after(mppi_ctx* c, const Plan& pl, uint64_t step, int spec_slot) {
  if (spec_slot < 0) return MPPI_OK;
  HIP_TRY(hipEventRecord(c->ns.ev_prev_roll, c->stream));
  return speculate_eps(c, pl, step, spec_slot, c->ns.ev_prev_roll);
}

// Finish arguments for `mode` (0: rank record, 1: finish; 1 becomes 2 with the deferred
// optimal rollout): claims the completion sequence number and the tail buffers of the
// next slot, ordering the context stream after the tail that last used them.
static int prepare_finish(mppi_ctx* c, const Plan& pl, const mppi_state& st, int mode, double* record_out,
                   FinishArgs& f, int& par) {
  // a server step's deferred tail (its completion word was seen) takes its slot first, so the slot
  // picked below is not the one it still has to read and write
  const int rc = flush_tail(c);
  if (rc) return rc;
  c->srv.cmd_live = false;
  fill_finish(c, pl, st, f);
  if (mode == 1 && c->tail.async) mode = 2;
  f.mode = mode;
  f.record_out = record_out;
  if (mode >= 1) {
    f.done = c->sb.done;
    f.seq = ++c->sb.seq;
    c->sb.wait_seq = c->sb.seq;
  }
  par = c->tail.pol.next();
  if (mode == 2) {
    f.tail_in = c->tail.in[par];
    f.tail_out = c->tail.host[par];
    // the tail of two steps ago used these buffers; in steady state it finished long ago
    // (it is shorter than a rollout kernel), so the cross-stream wait is rarely enqueued
    if (c->tail.pol.inflight[par]) {
      const hipError_t q = hipEventQuery(c->tail.ev[par]);
      if (q == hipErrorNotReady) HIP_TRY(hipStreamWaitEvent(c->stream, c->tail.ev[par], 0));
      else if (q != hipSuccess) return fail(MPPI_EHIP, std::string("tail: ") + hipGetErrorString(q));
      else c->tail.pol.done(par);
    }
  }
  return MPPI_OK;
}

// The deferred optimal rollout on a side stream: after the context stream's finish (event), or, for
// the resident server (its finish has published: f.clk set), at once.  The server's tails alternate
// over the tail and the noise stream: beside a server workgroup a tail takes about
// two step periods (~175 us against ~52 us alone at C3), so on one stream each waited for the one
// before it and the host for the slot.  More streams than the process's hardware queues
// (GPU_MAX_HW_QUEUES, 4 by default: torch's, the context's, the tail's and the noise stream's)
// share a queue, and a tail queued behind the resident server on the context's queue waited for it
// (measured with one stream per slot: every fourth command 66-102 us late).
static int enqueue_tail(mppi_ctx* c, const FinishArgs& f, int par) {
  const bool server = f.clk != nullptr;
  hipStream_t ts = (server && (par & 1)) ? c->ns.stream : c->tail.stream;
  if (!server) {
    HIP_TRY(hipEventRecord(c->tail.ev_fin_done, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->tail.stream, c->tail.ev_fin_done, 0));
  }
  if (c->tm.mode == 1) collect_tail_timing(c);  // (waits for the previous tail: mode 2 leaves the tail untimed)
  const int rc = timed_launch(c, c->tm.mode == 1, 4, ts, c->tm.tail_pending, [&] { return launch_tail(f, ts); });
  if (rc) return rc;
  HIP_TRY(hipEventRecord(c->tail.ev[par], ts));
  c->tail.ts[par] = ts;
  c->tail.pol.claim(par);
  return MPPI_OK;
}

int enqueue_finish(mppi_ctx* c, const Plan& pl, const mppi_state& st, const double* recs, int n,
                   int mode, double* record_out, bool timed) {
  FinishArgs f;
  int par = 0;
  int rc = prepare_finish(c, pl, st, mode, record_out, f, par);
  if (rc) return rc;
  f.recs = recs;
  f.n_recs = n;
  f.rec_m = recs == c->sb.nodes ? c->sb.rec_m : nullptr;  // this context's rollout records
  if (n > 1) {
    rc = ensure_nodes(c, n);
    if (rc) return rc;
    f.scratch0 = c->sb.scratch0;
    f.scratch1 = c->sb.scratch1;
  }
  // column-split finish (default): one launch, no partial-tree handoff between workgroups
  int cf_P = 0, cf_ncol = 0, cf_groups = 0;
  size_t cf_lds = 0;
  if (c->colfin && colfin_shape(n, H_of(c), &cf_P, &cf_ncol, &cf_groups, &cf_lds)) {
    f.level1 = c->sb.level1;
    f.level1_cnt = c->sb.level1_cnt;
    c->last.fin_kind = 1;
    c->last.fin_P = cf_P;
    c->last.fin_ncol = cf_ncol;
    c->last.fin_groups = cf_groups;
    const size_t lds = std::max(cf_lds, f.mode == 0 ? (size_t)0 : pl.fin_lds_bytes);
    rc = timed_launch(c, timed && c->tm.mode == 1, 2, c->stream, c->tm.fin_pending,
                      [&] { return launch_colfin(f, lds, c->stream, cf_P, cf_ncol, cf_groups); });
    if (rc) return rc;
    if (f.mode == 2) return enqueue_tail(c, f, par);
    return MPPI_OK;
  }
  // first tree level on ceil(n/16) workgroups (one per aligned group of 16 records)
  const int groups = n > 16 ? (n + 15) / 16 : 1;
  if (groups > 1) {
    rc = grow(c->sb.level1, (size_t)groups * E_of(c) * sizeof(double), c->stream);
    if (rc) return rc;
    f.level1 = c->sb.level1;
    f.level1_cnt = c->sb.level1_cnt;
  }
  c->last.fin_kind = 0;
  c->last.fin_P = n;
  c->last.fin_ncol = 0;
  c->last.fin_groups = groups;
  rc = timed_launch(c, timed && c->tm.mode == 1, 2, c->stream, c->tm.fin_pending, [&] {
    return launch_finish(f, f.mode == 0 ? pl.fin_tree_bytes : pl.fin_lds_bytes, c->stream, groups);
  });
  if (rc) return rc;
  if (f.mode == 2) return enqueue_tail(c, f, par);
  return MPPI_OK;
}

// The controls and velocities [0, 4H) of an output block.
static void fill_controls(const float* o, int H, mppi_outputs* out) {
  if (out->u1_opt) std::memcpy(out->u1_opt, o, H * sizeof(float));
  if (out->u2_opt) std::memcpy(out->u2_opt, o + H, H * sizeof(float));
  if (out->lin_vel) std::memcpy(out->lin_vel, o + 2 * H, H * sizeof(float));
  if (out->ang_vel) std::memcpy(out->ang_vel, o + 3 * H, H * sizeof(float));
}

static void fill_outputs(const float* o, int H, mppi_outputs* out) {
  fill_controls(o, H, out);
  if (out->traj_sim) std::memcpy(out->traj_sim, o + 4 * H, 3 * H * sizeof(float));
  if (out->heading_sim) std::memcpy(out->heading_sim, o + 7 * H, 3 * H * sizeof(float));
  if (out->left_wheel_sim) std::memcpy(out->left_wheel_sim, o + 10 * H, 3 * H * sizeof(float));
  if (out->right_wheel_sim) std::memcpy(out->right_wheel_sim, o + 13 * H, 3 * H * sizeof(float));
}

int copy_outputs(mppi_ctx* c, mppi_outputs* out) {
  const int H = H_of(c);
  int rc = wait_done(c);
  if (rc) {
    c->tail.pol.pending = false;  // a failed step's tail (if any) has nothing to merge or to launch
    c->tail.pol.deferred = false;
    return rc;
  }
  if (c->tail.async) {
    // controls + the first optimal-rollout row now; rows 1.. arrive with the tail
    const float* stage = c->sb.stage;
    collect_timing(c);
    c->sb.cur ^= 1;
    std::memcpy(c->sb.out_host.get(), stage, (size_t)4 * H * sizeof(float));
    if (out) {
      const float* o = stage;
      fill_controls(o, H, out);
      if (out->traj_sim) std::memcpy(out->traj_sim, o + 4 * H, 3 * sizeof(float));
      if (out->heading_sim) std::memcpy(out->heading_sim, o + 4 * H + 3, 3 * sizeof(float));
      if (out->left_wheel_sim) std::memcpy(out->left_wheel_sim, o + 4 * H + 6, 3 * sizeof(float));
      if (out->right_wheel_sim) std::memcpy(out->right_wheel_sim, o + 4 * H + 9, 3 * sizeof(float));
    }
    return MPPI_OK;
  }
  std::memcpy(c->sb.out_host.get(), c->sb.stage, (size_t)16 * H * sizeof(float));
  collect_timing(c);
  c->sb.cur ^= 1;  // the finish wrote the new nominal sequence into u_nom[cur^1]
  if (out) fill_outputs(c->sb.out_host.get(), H, out);
  return MPPI_OK;
}

static void remember(mppi_ctx* c, int proj, uint64_t step, int mode, const Plan& pl) {
  c->last.have = true;
  c->last.proj = proj;
  c->last.step = step;
  c->last.mode = mode;
  c->last.state = c->sb.st;
  c->last.nominal = c->sb.cur;  // nominal buffer the rollout read (before the swap)
  c->last.plan = pl;
}

// ---- resident step server (mppi_step_server_kernel) ----
// Sampled steps of the role-split plan whose records fit the column-split finish in the rollout
// workgroups (C1-C3).  Per step the host waits (normally not at all) for the step's normals and the
// tail slot it reuses, writes the command (state, slots, nominal buffer, the slot for the normals of
// step + 2 that the server's noise phase generates, then seq), launches the server if it is not
// running, launches the PREVIOUS step's deferred optimal rollout (flush_tail: its completion word has
// been seen) and spins on the completion word.  This step's tail stays on the host (tail.pol.deferred)
// until the next step, sync_tail (get_outputs and every call that quiesces before reading the DEM)
// or prepare_finish (any separate-launch finish: it takes the slot after the deferred one).  No launch and no kernel boundary on the step's path: the gap between two steps
// is the host's round trip (completion word seen -> next command) plus one poll of pinned memory.
// MPPI_HOST_TRACE marks of a step: 0 entry, 1 normals ready, 2 tail slot free (server), 3 command
// posted / launches enqueued, 4 side launches done (the previous tail), 5 completion seen + copies
static void trace_mark(mppi_ctx* c, int k) {
  if (c && c->tm.trace) c->tm.tr_m[k] = now_us();
}

static bool server_shape(const mppi_ctx* c, const Plan& pl, int mode, int* P, int* ncol, int* groups, size_t* lds) {
  // (every workgroup of the server must be resident at once: one rollout block per CU at most)
  // (beta > 0: the generator's serial form is a whole step's Philox blocks per wave, which the
  // server's static shares of single blocks cannot hold: such a plan runs as separate launches)
  if (c->samp.beta > 0.0f) return false;
  if (!c->srv.resident || mode != 0 || !pl.roles || !c->colfin || c->tm.mode != 0 || pl.blocks < 1 ||
      pl.blocks > std::max(c->num_cus, 1))
    return false;
  size_t cf_lds = 0;
  // the finish runs in the workgroups holding the last `groups` tickets: at most one per rollout workgroup
  if (!colfin_shape(pl.blocks, H_of(c), P, ncol, groups, &cf_lds, pl.blocks)) return false;
  *lds = std::max({pl.lds_bytes, cf_lds, pl.fin_lds_bytes});
  return *lds + 256 <= kLdsBytes;  // + the kernel's static words (command, ticket)
}

static int server_step(mppi_ctx* c, int proj, uint64_t step, const Plan& pl, int P, int ncol, int groups, size_t lds) {
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  if (c->srv.running && proj != c->srv.proj) post_stop(c);  // (the next launch queues behind it)
  // (first step: the buffers are allocated before the server holds pointers to them)
  int rc = MPPI_OK;
  if (c->sb.nodes_cap < (size_t)pl.blocks * E_of(c) || c->ns.cap < (size_t)pl.blocks * 2 * H_of(c) * 256)
    rc = quiesce(c);
  if (!rc) rc = ensure_nodes(c, pl.blocks);
  if (rc) return rc;
  int slot = 0, noise_slot = -1;
  const uint64_t nb = (uint64_t)((H_of(c) + 1) / 2);  // Philox blocks per trajectory and step
  // a step whose normals no slot holds (first step, a jump of the step counter): the server may still
  // be writing normals of a later step in its last noise phase, so it is stopped before any slot is
  // regenerated
  if (!c->ns.pol.holds(step) && (rc = quiesce(c))) return rc;
  rc = eps_for_step(c, pl, step, c->ns.stream, true, &slot);
  if (rc) return rc;
  trace_mark(c, 1);
  // normals of step + 1 (normally generated by the previous step's noise phase; else now, on the
  // noise stream beside this step) and of step + 2 (by this step's noise phase, in the server)
  // the server's noise phase runs mostly in the workgroups outside the finish: with fewer than a
  // quarter of them, or fewer than two (few records: every rollout workgroup may hold a finish
  // column) the noise kernel does it
  const bool srv_noise = pl.blocks - groups >= 2 &&
                         (int64_t)(pl.blocks - groups) * 4 >= (int64_t)pl.blocks;
  for (int d = 1; d <= 2; ++d) {
    const uint64_t target = step + (uint64_t)d;
    if (c->ns.pol.holds(target)) continue;
    const int v = c->ns.pol.victim(slot, step);
    if (v < 0) return fail(MPPI_ESTATE, "no free noise slot");
    if (d == 1 || !srv_noise) {
      HIP_TRY(launch_noise(c->p.seed, target * nb, c->p.k_offset, pl.blocks, H_of(c), c->ns.buf[v], c->ns.stream,
                           noise_groups(c), device_plan(c->samp)));
      HIP_TRY(hipEventRecord(c->ns.ev[v], c->ns.stream));
      c->ns.pol.mark_pending(v, target);
    } else {
      // complete before step + 2 can be commanded: every workgroup ends its noise phase before its
      // rollout of step + 1, whose records the completion of step + 1 needs
      noise_slot = v;
      c->ns.pol.mark_ready(v, target);
    }
  }
  const int par = c->tail.pol.next();
  if (c->tail.async && c->tail.pol.inflight[par]) {  // the tail of kTailSlots steps ago: long done
    HIP_TRY(hipEventSynchronize(c->tail.ev[par]));
    c->tail.pol.done(par);
  }
  trace_mark(c, 2);
  const unsigned seq = ++c->sb.seq;
  c->sb.wait_seq = seq;
  // the command: every word travels with the step's seq as its tag (cmd_post below)
  ServerCmd d;
  std::memset(&d, 0, sizeof(d));
  state_fields(c->p, c->sb.st, d);
  d.eps_slot = slot;
  d.cur = c->sb.cur;
  d.tail_slot = par;
  d.mode = c->tail.async ? 2 : 1;
  d.noise_slot = noise_slot;
  c->srv.cmd_noise = noise_slot;
  const uint64_t nbase = (step + 2) * nb;
  d.noise_n_base_lo = (unsigned)nbase;
  d.noise_n_base_hi = (unsigned)(nbase >> 32);
  // a server idle for more than half its limit (since its last step completed) may be leaving: stop
  // it and start a fresh one behind it.  This is checked after the host's waits above, right before
  // the command is posted; a head that leaves anyway (a slower host) never relays the command, and
  // wait_done relaunches the server with it
  if (c->srv.running && now_us() - c->srv.last_us > 0.5 * (double)c->srv.idle_us) post_stop(c);
  cmd_post(c->srv.cmd, d, seq);
  c->srv.pl = pl;
  c->srv.P = P;
  c->srv.ncol = ncol;
  c->srv.groups = groups;
  c->srv.lds = lds;
  c->srv.proj = proj;
  c->srv.cmd_live = true;
  if (!c->srv.running) {
    rc = launch_server(c, seq);
    if (rc) return rc;
  }
  c->srv.last_us = now_us();
  trace_mark(c, 3);
  ++c->srv.steps;
  c->last.fin_kind = 1;
  c->last.fin_P = P;
  c->last.fin_ncol = ncol;
  c->last.fin_groups = groups;
  rc = flush_tail(c);  // the previous step's tail (its outputs were published before this call)
  if (rc) return rc;
  if (c->tail.async) {  // rows 1.. of the optimal rollout: launched once this step has published
    FinishArgs& f = c->tail.def;
    fill_finish(c, pl, c->sb.st, f);
    f.mode = 2;
    f.seq = seq;
    f.tail_in = c->tail.in[par];
    f.tail_out = c->tail.host[par];
    f.clk = c->sb.clk;
    c->tail.pol.deferred = true;
    c->tail.pol.def_slot = par;
  }
  trace_mark(c, 4);
  return MPPI_OK;
}

// The launches of one step (rollout + finish + tail) outside the server.
static int enqueue_step(mppi_ctx* c, int proj, uint64_t step, int mode, const Plan& pl) {
  int spec = -1;
  int rc = enqueue_rollout(c, proj, step, mode, pl, c->sb.u_nom[c->sb.cur], c->sb.st, nullptr, &spec);
  if (rc) return rc;
  trace_mark(c, 3);
  rc = enqueue_finish(c, pl, c->sb.st, c->sb.nodes, pl.blocks, 1, nullptr, true);
  if (rc) return rc;
  return speculate_after(c, pl, step, spec);
}

static int step_impl(mppi_ctx* c, int proj, uint64_t step, int mode, mppi_outputs* out) {
  int rc = check_ready(c);
  if (rc) return rc;
  trace_mark(c, 0);
  const Plan pl = make_plan(c);
  int sP = 0, scol = 0, sgroups = 0;
  size_t slds = 0;
  bool resident = server_shape(c, pl, mode, &sP, &scol, &sgroups, &slds);
  const double now = now_us(), half = 0.5 * (double)c->srv.idle_us;
  const bool back_to_back = c->srv.last_return_us > 0 && now - c->srv.last_return_us <= half;
  c->srv.b2b_calls = back_to_back ? c->srv.b2b_calls + 1 : 0;
  c->ns.late = c->ns.after < 0 ? !back_to_back : c->ns.after == 1;
  if (resident && c->srv.resident == 1) {
    // the caller's cadence: a call more than half the idle limit after the last step returned (a
    // simulator frame) runs as separate launches, and a server that has been idle that long is told
    // to leave (the launches queue behind it); back-to-back calls keep the server, and start one when
    // the last step ran on a server (stopped by another call since, e.g. a synchronize) or the call is
    // the second back-to-back one in a row (a lone back-to-back call after a frame-cadence step would
    // pay a server launch for one step: separate launches are cheaper there)
    if (c->srv.running ? now - c->srv.last_us > half : !(back_to_back && (c->last.resident || c->srv.b2b_calls >= 2))) {
      post_stop(c);
      resident = false;
      ++c->srv.cadence_steps;
    }
  }
  if (!resident) {
    post_stop(c);  // (stream order: these launches run after it retired)
    rc = flush_tail(c);
    if (rc) return rc;
  }
  rc = resident ? server_step(c, proj, step, pl, sP, scol, sgroups, slds) : enqueue_step(c, proj, step, mode, pl);
  if (rc) return rc;
  c->last.resident = resident;
  remember(c, proj, step, mode, pl);
  trace_mark(c, 4);
  rc = copy_outputs(c, out);
  // A server step that did not complete published nothing and changed no state (wait_done stopped
  // the server, waited for it to retire and re-armed its counters): this step again as separate
  // launches.  Its finish gave up (1: the rollout workgroups could not all get CUs within the wait
  // bound, e.g. beside another process's kernels): counted, the server stays the schedule.  A fresh
  // launch retired without serving its first command (2): it cannot run here, separate launches from
  // now on.  (A server that left on its idle limit as the command was posted is neither: wait_done
  // relaunched it.)
  if (resident && rc == MPPI_EHIP && (c->srv.fail_kind == 1 || c->srv.fail_kind == 2)) {
    if (c->srv.fail_kind == 2) {
      if (!c->srv.warned)
        std::fprintf(stderr, "mppi: the resident step server could not run here; using separate launches\n");
      c->srv.warned = true;
      c->srv.resident = 0;
    } else {
      ++c->srv.fallbacks;
    }
    c->last.resident = false;
    rc = enqueue_step(c, proj, step, mode, pl);
    if (rc) return rc;
    rc = copy_outputs(c, out);
  }
  c->srv.last_return_us = now_us();
  if (c->tm.trace) {  // marks a schedule does not set (separate launches: 1, 2) take the one before
    c->tm.tr_m[5] = now_us();
    for (int k = 1; k < 6; ++k) c->tm.tr_m[k] = std::max(c->tm.tr_m[k], c->tm.tr_m[k - 1]);
    if (c->tm.tr_prev > 0) {
      c->tm.tr_sum[0] += c->tm.tr_m[0] - c->tm.tr_prev;
      for (int k = 1; k < 6; ++k) c->tm.tr_sum[k] += c->tm.tr_m[k] - c->tm.tr_m[k - 1];
      std::memcpy(c->tm.tr_log[c->tm.tr_n++ & 7], c->tm.tr_m, sizeof(c->tm.tr_m));
    }
    c->tm.tr_prev = c->tm.tr_m[5];
    std::memset(c->tm.tr_m, 0, sizeof(c->tm.tr_m));
  }
  return rc;
}

}  // namespace capi
}  // namespace mppi

extern "C" {

int mppi_abi_version(void) { return MPPI_ABI_VERSION; }

const char* mppi_last_error(void) { return g_err.c_str(); }

int mppi_create(const mppi_params* params, int32_t device, mppi_ctx** out) {
  if (!params || !out) return fail(MPPI_EINVAL, "null argument");
  *out = nullptr;
  const mppi_params& p = *params;
  if (p.num_iterations < 1 || p.num_iterations > 255)
    return fail(MPPI_EINVAL, "num_iterations must be in [1, 255]");
  if (p.num_trajectories < 0 || p.num_trajectories > ((int64_t)1 << 31) * 64)
    return fail(MPPI_EINVAL, "num_trajectories out of range");
  if (p.k_offset < 0) return fail(MPPI_EINVAL, "k_offset must be >= 0");
  if (!(p.temperature > 0.0f)) return fail(MPPI_EINVAL, "temperature must be > 0");
  if (!(p.dt > 0.0f)) return fail(MPPI_EINVAL, "dt must be > 0");
  if (p.robot_radius == 0.0f) return fail(MPPI_EINVAL, "robot_radius must be non-zero");
  int ndev = 0;
  HIP_TRY(hipGetDeviceCount(&ndev));
  if (device < 0 || device >= ndev)
    return fail(MPPI_EHIP, "device " + std::to_string(device) + " not available (" +
                               std::to_string(ndev) + " HIP devices)");
  HIP_TRY(hipSetDevice(device));
  std::unique_ptr<mppi_ctx> owner(new mppi_ctx());  // a failed create just returns: the parts release what they hold
  mppi_ctx* c = owner.get();
  c->p = p;
  c->device = device;
  {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0)
      c->num_cus = cus;
  }
  // runtime environment knobs: MPPI_HOST_TRACE, MPPI_ROLES, MPPI_RESIDENT (and
  // MPPI_GROUP_RCCL for groups)
  if (const char* e = std::getenv("MPPI_HOST_TRACE")) c->tm.trace = std::atoi(e) != 0;
  if (const char* e = std::getenv("MPPI_ROLES")) c->roles = std::atoi(e) != 0;
  if (const char* e = std::getenv("MPPI_RESIDENT")) c->srv.resident = std::min(std::max(std::atoi(e), 0), 2);
  const int H = p.num_iterations;
  const size_t cost_bytes = std::max<int64_t>(p.num_trajectories, 1) * sizeof(float);
  StepBuffers& sb = c->sb;
  // the rollout stream outranks the speculative noise stream at dispatch
  if (hipDeviceGetStreamPriorityRange(&c->prio_least, &c->prio_greatest) != hipSuccess)
    return fail(MPPI_EHIP, "hipDeviceGetStreamPriorityRange failed");
  if (c->stream.create(hipStreamNonBlocking, c->prio_greatest)) return fail(MPPI_EHIP, "hipStreamCreate failed");
  if (sb.u_nom[0].alloc(2 * H * sizeof(float)) || sb.u_nom[1].alloc(2 * H * sizeof(float)) || sb.cost.alloc(cost_bytes) ||
      sb.stage.alloc(16 * H * sizeof(float)) || sb.done.alloc(64) || c->cdiv_bad.alloc(sizeof(unsigned)) ||
      sb.level1_cnt.alloc(128) ||  // [0]: finish handoff, [16]: the server's record count
      sb.uopt.alloc((size_t)2 * H * sizeof(unsigned long long)) || c->srv.cmd.alloc(sizeof(ServerCmdWire)) ||
      c->srv.relay.alloc(sizeof(ServerCmdWire)) || sb.clk.alloc(kClkWords * sizeof(uint64_t)))
    return fail(MPPI_EHIP, "device allocation failed");
  for (int i = 0; i < kTailSlots; ++i)
    if (c->tail.in[i].alloc(3 * H * sizeof(float)) || c->tail.host[i].alloc(12 * H * sizeof(float)) ||
        c->tail.ev[i].create(hipEventDisableTiming))
      return fail(MPPI_EHIP, "tail slot allocation failed");
  if (hipMemset(sb.u_nom[0], 0, 2 * H * sizeof(float)) != hipSuccess ||
      hipMemset(sb.u_nom[1], 0, 2 * H * sizeof(float)) != hipSuccess ||
      hipMemset(sb.cost, 0, cost_bytes) != hipSuccess ||
      hipMemset(c->srv.relay, 0, sizeof(ServerCmdWire)) != hipSuccess ||
      hipMemset(sb.clk, 0, kClkWords * sizeof(uint64_t)) != hipSuccess)
    return fail(MPPI_EHIP, "hipMemset failed");
  for (auto& e : c->tm.ev)
    if (e.create()) return fail(MPPI_EHIP, "hipEventCreate failed");
  if (c->tail.ev_fin_done.create(hipEventDisableTiming) || c->tail.stream.create(hipStreamNonBlocking) ||
      c->ns.stream.create(hipStreamNonBlocking, c->prio_least) || c->ns.ev_prev_roll.create(hipEventDisableTiming) ||
      c->tm.ev_side[0].create(hipEventDisableTiming) || c->tm.ev_side[1].create(hipEventDisableTiming))
    return fail(MPPI_EHIP, "side stream / event creation failed");
  for (auto& e : c->ns.ev)
    if (e.create(hipEventDisableTiming)) return fail(MPPI_EHIP, "side stream / event creation failed");
  sb.out_host.reset(new float[16 * H]());
  std::memset(sb.stage, 0, 16 * H * sizeof(float));
  *sb.done = 0;
  std::memset(c->srv.cmd, 0, sizeof(ServerCmdWire));
  if (hipMemset(sb.level1_cnt, 0, 128) != hipSuccess ||
      hipMemset(sb.uopt, 0, (size_t)2 * H * sizeof(unsigned long long)) != hipSuccess)
    return fail(MPPI_EHIP, "hipMemset failed");
  if (hipDeviceSynchronize() != hipSuccess) return fail(MPPI_EHIP, "device sync failed");
  *out = owner.release();
  return MPPI_OK;
}

void mppi_destroy(mppi_ctx* c) {
  if (!c) return;
  (void)quiesce(c);
  if (c->tm.trace && c->tm.tr_n > 0) {
    static const char* ph[6] = {"caller", "normals wait", "tail slot wait", "command / launches", "side launches",
                                "completion + copies"};
    std::fprintf(stderr, "mppi host trace (us/step over %ld steps; server launches %ld, relaunches %ld):", c->tm.tr_n,
                 (long)c->srv.launches, (long)c->srv.relaunches);
    for (int k = 0; k < 6; ++k) std::fprintf(stderr, "  %s %.1f", ph[k], c->tm.tr_sum[k] / c->tm.tr_n);
    std::fprintf(stderr, "\n");
    for (long r = std::max(0L, c->tm.tr_n - 8); r < c->tm.tr_n; ++r) {  // the last 8 steps' marks, from entry
      const double* lg = c->tm.tr_log[r & 7];
      std::fprintf(stderr, "  host step %ld:", r);
      for (int k = 1; k < 6; ++k) std::fprintf(stderr, " %+7.1f", lg[k] - lg[0]);
      std::fprintf(stderr, "\n");
    }
  }
  hipSetDevice(c->device);
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->tail.stream) hipStreamSynchronize(c->tail.stream);
  if (c->ns.stream) hipStreamSynchronize(c->ns.stream);
  delete c;  // the parts release their buffers, events and streams
}

int mppi_set_stream(mppi_ctx* c, void* s) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  int rc = sync_tail(c);
  if (rc) return rc;
  if (s) c->stream.borrow((hipStream_t)s);  // (an owned stream is destroyed as its handle lets go of it)
  else HIP_TRY(c->stream.create(hipStreamNonBlocking, c->prio_greatest));
  return MPPI_OK;
}

static int check_grid(int32_t rows, int32_t cols, float res) {
  if (rows < 2 || cols < 2) return fail(MPPI_EINVAL, "DEM must be at least 2x2");
  if (!(res > 0.0f)) return fail(MPPI_EINVAL, "DEM resolution must be > 0");
  if ((int64_t)rows * cols >= ((int64_t)1 << 29))  // kernels address cells with 32-bit byte offsets
    return fail(MPPI_EINVAL, "DEM larger than 2^29 cells");
  if (((int64_t)rows + 1) * ((int64_t)cols + 1) * 16 >= ((int64_t)1 << 32))  // the normal table, ditto
    return fail(MPPI_EINVAL, "DEM normal table above 4 GiB ((rows+1)*(cols+1) >= 2^28)");
  if (rows > (1 << 24) || cols > (1 << 24))  // cell bounds are clamped as exact floats
    return fail(MPPI_EINVAL, "DEM dimension above 2^24");
  return MPPI_OK;
}

// The DEM's per-cell normal table (read by the rollout chain instead of four corners +
// a normalisation per step); rebuilt whenever the DEM is set.  Ends synchronised.
static int build_normal_table(mppi_ctx* c) {
  const int rc = grow(c->dem.ntab, ((size_t)c->dem.rows + 1) * ((size_t)c->dem.cols + 1) * sizeof(float4), c->stream);
  if (rc) return rc;
  HIP_TRY(launch_normal_table(c->dem.Z, c->dem.rows, c->dem.cols, c->dem.res, c->dem.ntab, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_set_dem(mppi_ctx* c, const float* z, int32_t rows, int32_t cols, float x_min, float y_min,
                 float resolution) {
  if (!c || !z) return fail(MPPI_EINVAL, "null argument");
  return install_dem(c, rows, cols, x_min, y_min, resolution, [&](float* dst) {
    HIP_TRY(hipMemcpyAsync(dst, z, (size_t)rows * cols * sizeof(float), hipMemcpyHostToDevice, c->stream));
    return (int)MPPI_OK;
  });
}

// mppi_set_dem from the quiesce on.  `fill(dst)` enqueues the heights into the context's own DEM
// buffer on the context stream (mppi_set_dem: the copy from the host; mppi_build_dem: the product
// kernel); the stream is waited for before the geometry changes.
extern "C++" int mppi::capi::install_dem(mppi_ctx* c, int32_t rows, int32_t cols, float x_min, float y_min,
                                         float resolution, const std::function<int(float*)>& fill) {
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = check_grid(rows, cols, resolution);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  rc = sync_tail(c);  // a deferred optimal rollout may still read the DEM
  if (rc) return rc;
  const size_t bytes = (size_t)rows * cols * sizeof(float);
  if (!c->dem.Z.owned() || bytes > c->dem.Z.cap()) {  // (a borrowed DEM is let go of, not written into)
    HIP_TRY(hipStreamSynchronize(c->stream));
    HIP_TRY(c->dem.Z.alloc(bytes));
  }
  rc = fill(c->dem.Z);
  if (rc) return rc;
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->dem.rows = rows;
  c->dem.cols = cols;
  c->dem.x_min = x_min;
  c->dem.y_min = y_min;
  c->dem.res = resolution;
  rc = build_normal_table(c);
  if (rc) return rc;
  return verified_reciprocal(c, resolution, &c->dem.rinv_res);
}

int mppi_set_dem_device(mppi_ctx* c, const float* z, int32_t rows, int32_t cols, float x_min,
                        float y_min, float resolution) {
  if (!c || !z) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = check_grid(rows, cols, resolution);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // the DEM's writer may be on any stream of the device
  rc = sync_tail(c);
  if (rc) return rc;
  c->dem.Z.borrow(const_cast<float*>(z));  // (frees a DEM of mppi_set_dem)
  c->dem.rows = rows;
  c->dem.cols = cols;
  c->dem.x_min = x_min;
  c->dem.y_min = y_min;
  c->dem.res = resolution;
  rc = build_normal_table(c);
  if (rc) return rc;
  return verified_reciprocal(c, resolution, &c->dem.rinv_res);
}

int mppi_dem_updated(mppi_ctx* c) {
  if (!c) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (!c->dem.Z || c->dem.rows <= 0) return fail(MPPI_EINVAL, "no DEM bound");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // the in-place write may be on any stream of the device
  const int rc = sync_tail(c);      // a deferred optimal rollout may still read the table
  if (rc) return rc;
  return build_normal_table(c);
}

int mppi_set_costmap(mppi_ctx* c, const float* cm, int32_t size, float half_width, float resolution) {
  if (!c || !cm) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (size < 1) return fail(MPPI_EINVAL, "costmap size must be >= 1");
  if (!(resolution > 0.0f)) return fail(MPPI_EINVAL, "costmap resolution must be > 0");
  HIP_TRY(hipSetDevice(c->device));
  const size_t bytes = (size_t)size * size * sizeof(float);
  const int rc = grow(c->cmap.cm, bytes, c->stream);
  if (rc) return rc;
  HIP_TRY(hipMemcpyAsync(c->cmap.cm, cm, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  c->cmap.size = size;
  c->cmap.hw = half_width;
  c->cmap.res = resolution;
  return verified_reciprocal(c, resolution, &c->cmap.rinv_res);
}

int mppi_set_state(mppi_ctx* c, const mppi_state* s) {
  if (!c || !s) return fail(MPPI_EINVAL, "null argument");
  c->sb.st = *s;
  c->sb.have_state = true;
  return MPPI_OK;
}

int mppi_set_nominal(mppi_ctx* c, const float* u1, const float* u2) {
  if (!c || !u1 || !u2) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  const int H = H_of(c);
  HIP_TRY(hipMemcpyAsync(c->sb.u_nom[c->sb.cur], u1, H * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->sb.u_nom[c->sb.cur] + H, u2, H * sizeof(float), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_get_nominal(mppi_ctx* c, float* u1, float* u2) {
  if (!c || !u1 || !u2) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  const int H = H_of(c);
  HIP_TRY(hipMemcpyAsync(u1, c->sb.u_nom[c->sb.cur], H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(u2, c->sb.u_nom[c->sb.cur] + H, H * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_step(mppi_ctx* c, int32_t proj, uint64_t step, mppi_outputs* out) {
  return step_impl(c, proj, step, 0, out);
}

int mppi_step_injected(mppi_ctx* c, int32_t proj, const float* u1, const float* u2,
                       mppi_outputs* out) {
  if (!c || !u1 || !u2) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)std::max<int64_t>(c->p.num_trajectories, 1) * H_of(c);
  if (!c->sb.inj1) {
    HIP_TRY(c->sb.inj1.alloc(n * sizeof(float)));
    HIP_TRY(c->sb.inj2.alloc(n * sizeof(float)));
  }
  const size_t bytes = (size_t)c->p.num_trajectories * H_of(c) * sizeof(float);
  HIP_TRY(hipMemcpyAsync(c->sb.inj1, u1, bytes, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->sb.inj2, u2, bytes, hipMemcpyHostToDevice, c->stream));
  return step_impl(c, proj, 0, 1, out);
}

int64_t mppi_record_len(mppi_ctx* c) { return c ? E_of(c) : -1; }

int mppi_step_partial(mppi_ctx* c, int32_t proj, uint64_t step, double* record_dev) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = check_ready(c);
  if (rc) return rc;
  if (!record_dev) return fail(MPPI_EINVAL, "null record buffer");
  const Plan pl = make_plan(c);
  c->last.resident = false;
  int spec = -1;
  c->ns.late = c->ns.after == 1;  // (a group's or rank's partial steps: back to back)
  rc = enqueue_rollout(c, proj, step, 0, pl, c->sb.u_nom[c->sb.cur], c->sb.st, nullptr, &spec);
  if (rc) return rc;
  remember(c, proj, step, 0, pl);
  rc = enqueue_finish(c, pl, c->sb.st, c->sb.nodes, pl.blocks, 0, record_dev, false);
  if (rc) return rc;
  return speculate_after(c, pl, step, spec);
}

int mppi_step_finish(mppi_ctx* c, const double* records_dev, int32_t n, mppi_outputs* out) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = check_ready(c);
  if (rc) return rc;
  if (!records_dev || n < 1) return fail(MPPI_EINVAL, "records required");
  const Plan pl = c->last.have ? c->last.plan : make_plan(c);
  rc = enqueue_finish(c, pl, c->sb.st, records_dev, n, 1, nullptr, true);
  if (rc) return rc;
  return copy_outputs(c, out);
}

int mppi_get_costs(mppi_ctx* c, float* costs, int64_t n) {
  if (!c || !costs) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (n < 0 || n > c->p.num_trajectories) return fail(MPPI_EINVAL, "n out of range");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(costs, c->sb.cost, n * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_set_critics(mppi_ctx* c, const mppi_critics* k) {
  if (!c || !k) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;  // the next server launch carries the set
  const std::string err = critics_error(*k, H_of(c));
  if (!err.empty()) return fail(MPPI_EINVAL, "set_critics: " + err);
  c->crit = *k;
  return MPPI_OK;
}

int mppi_get_critics(mppi_ctx* c, mppi_critics* out) {
  if (!c || !out) return fail(MPPI_EINVAL, "null argument");
  *out = c->crit;
  return MPPI_OK;
}

int mppi_set_sampling(mppi_ctx* c, const mppi_sampling* s) {
  if (!c || !s) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;  // the next server launch carries the plan
  const std::string err = sampling_error(*s, c->p.k_offset);
  if (!err.empty()) return fail(MPPI_EINVAL, "set_sampling: " + err);
  // the normals generated ahead were drawn under the old plan: no slot holds a step any more (fills
  // still in flight are waited for before their slot is written again, eps_for_step)
  c->ns.pol.forget_steps();
  c->samp = *s;
  return MPPI_OK;
}

int mppi_get_sampling(mppi_ctx* c, mppi_sampling* out) {
  if (!c || !out) return fail(MPPI_EINVAL, "null argument");
  *out = c->samp;
  return MPPI_OK;
}

int mppi_dump_rollouts(mppi_ctx* c, float* traj, float* hv, float* lw, float* rw, float* v, float* w,
                       float* u1, float* u2) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = check_ready(c);
  if (rc) return rc;
  if (!c->last.have) return fail(MPPI_ESTATE, "no step to dump");
  const size_t KH = (size_t)c->p.num_trajectories * H_of(c);
  if (KH == 0) return MPPI_OK;
  float* host[8] = {traj, hv, lw, rw, v, w, u1, u2};
  const size_t cnt[8] = {3 * KH, 3 * KH, 3 * KH, 3 * KH, KH, KH, KH, KH};
  DeviceBuf<float> dev[8];
  int out_rc = MPPI_OK;
  for (int i = 0; i < 8 && out_rc == MPPI_OK; ++i)
    if (host[i] && dev[i].alloc(cnt[i] * sizeof(float)))
      out_rc = fail(MPPI_EHIP, "dump allocation failed");
  if (out_rc == MPPI_OK) {
    RolloutArgs d;
    std::memset(&d, 0, sizeof(d));
    d.d_traj = dev[0];
    d.d_hv = dev[1];
    d.d_lw = dev[2];
    d.d_rw = dev[3];
    d.d_v = dev[4];
    d.d_w = dev[5];
    d.d_u1 = dev[6];
    d.d_u2 = dev[7];
    // re-run the last step (deterministic: costs/records are rewritten with identical values)
    out_rc = enqueue_rollout(c, c->last.proj, c->last.step, c->last.mode, c->last.plan,
                             c->sb.u_nom[c->last.nominal], c->last.state, &d);
    for (int i = 0; i < 8 && out_rc == MPPI_OK; ++i)
      if (host[i] && hipMemcpyAsync(host[i], dev[i], cnt[i] * sizeof(float), hipMemcpyDeviceToHost,
                                    c->stream) != hipSuccess)
        out_rc = fail(MPPI_EHIP, "dump copy failed");
    if (out_rc == MPPI_OK && hipStreamSynchronize(c->stream) != hipSuccess)
      out_rc = fail(MPPI_EHIP, "dump sync failed");
  }
  return out_rc;
}

int mppi_set_option(mppi_ctx* c, const char* name, int64_t value) {
  if (!c || !name) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  const std::string n(name);
  if (n == "resident") {  // the resident step server: 1 for back-to-back calls (default), 2 always, 0 never
    if (value < 0 || value > 2) return fail(MPPI_EINVAL, "resident must be 0, 1 or 2");
    c->srv.resident = (int)value;
    return MPPI_OK;
  }
  if (n == "resident_idle_us") {  // how long an idle server stays resident
    if (value < 100 || value > 1000000) return fail(MPPI_EINVAL, "resident_idle_us must be in [100, 1e6]");
    c->srv.idle_us = (uint64_t)value;
    return MPPI_OK;
  }
  if (n == "record_tree_finish") {  // 1: the record-tree finish (mppi_finish_kernel) at any record count
    c->colfin = value == 0;
    return MPPI_OK;
  }
  if (n == "verified_reciprocal") {  // test hook: 0 puts every cell index on the IEEE division (rinv_res = 0)
    if (value < 0 || value > 1) return fail(MPPI_EINVAL, "verified_reciprocal must be 0 or 1");
    HIP_TRY(hipSetDevice(c->device));
    c->use_cdiv = value != 0;
    if (c->dem.Z)
      if (int rc = verified_reciprocal(c, c->dem.res, &c->dem.rinv_res)) return rc;
    if (c->cmap.cm)
      if (int rc = verified_reciprocal(c, c->cmap.res, &c->cmap.rinv_res)) return rc;
    return MPPI_OK;
  }
  if (n == "server_exit_after") {  // test hook: the next server launch's head leaves after this many commands
    if (value < 0 || value > 1000000) return fail(MPPI_EINVAL, "server_exit_after must be in [0, 1e6]");
    c->srv.exit_after = (unsigned)value;
    return MPPI_OK;
  }
  if (n == "eps_after") {  // the next steps' normals after the finish (1), the rollout (0), by cadence (-1)
    if (value < -1 || value > 1) return fail(MPPI_EINVAL, "eps_after must be -1, 0 or 1");
    c->ns.after = (int)value;
    return MPPI_OK;
  }
  if (n == "finish_wait_ticks") {  // the server finish's record wait bound (100 MHz ticks; 0: give up at once)
    if (value < 0) return fail(MPPI_EINVAL, "finish_wait_ticks must be >= 0");
    c->srv.fin_wait_ticks = (uint64_t)value;
    return MPPI_OK;
  }
  return fail(MPPI_EINVAL, "unknown option '" + n + "'");
}

int mppi_set_timing(mppi_ctx* c, int32_t enable) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  int rc = sync_tail(c);
  if (rc) return rc;
  if (enable < 0 || enable > 2) return fail(MPPI_EINVAL, "timing mode must be 0, 1 or 2");
  c->tm.mode = enable;
  c->tm.t_roll = c->tm.t_fin = c->tm.t_tail = 0.0;
  c->tm.launches = c->tm.tail_launches = 0;
  c->tm.roll_pending = c->tm.fin_pending = c->tm.tail_pending = false;
  return MPPI_OK;
}

int mppi_get_tail_timing(mppi_ctx* c, double* tail_ms, int64_t* n) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  int rc = sync_tail(c);
  if (rc) return rc;
  if (tail_ms) *tail_ms = c->tm.t_tail;
  if (n) *n = c->tm.tail_launches;
  return MPPI_OK;
}

int mppi_set_async_tail(mppi_ctx* c, int32_t enable) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  int rc = sync_tail(c);
  if (rc) return rc;
  c->tail.async = enable != 0;
  return MPPI_OK;
}

int mppi_get_outputs(mppi_ctx* c, mppi_outputs* out) {
  if (!c || !out) return fail(MPPI_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  int rc = sync_tail(c);
  if (rc) return rc;
  fill_outputs(c->sb.out_host.get(), H_of(c), out);
  return MPPI_OK;
}

int mppi_get_timing(mppi_ctx* c, double* roll, double* fin, int64_t* n) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (roll) *roll = c->tm.t_roll;
  if (fin) *fin = c->tm.t_fin;
  if (n) *n = c->tm.launches;
  return MPPI_OK;
}

int mppi_get_server_time(mppi_ctx* c, double* roll_us, double* step_us, int64_t* steps) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  HIP_TRY(hipSetDevice(c->device));
  uint64_t v[4] = {0, 0, 0, 0};
  // (a side stream: the context stream may hold the running server)
  HIP_TRY(hipMemcpyAsync(v, c->sb.clk + kClkSums, sizeof(v), hipMemcpyDeviceToHost, c->ns.stream));
  HIP_TRY(hipStreamSynchronize(c->ns.stream));
  if (roll_us) *roll_us = (double)v[0] / 100.0;
  if (step_us) *step_us = (double)v[2] / 100.0;
  if (steps) *steps = (int64_t)std::min(v[1], v[3]);
  return MPPI_OK;
}

int mppi_get_chain_clock(mppi_ctx* c, double* out, int32_t n) {
  if (!c || !out) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  std::vector<uint64_t> all((size_t)kClkWords, 0);
  HIP_TRY(hipMemcpy(all.data(), c->sb.clk, all.size() * sizeof(uint64_t), hipMemcpyDeviceToHost));
  const uint64_t* v = all.data();
  // per-workgroup start / end of the last role-split rollout (its plan's blocks)
  const int nb = std::min(c->last.plan.roles ? c->last.plan.blocks : 0, kClkBlocks);
  uint64_t s_lo = UINT64_MAX, s_hi = 0, e_lo = UINT64_MAX, e_hi = 0;
  for (int b = 0; b < nb; ++b) {
    const uint64_t s0 = v[kClkBase + 2 * b], e0 = v[kClkBase + 2 * b + 1];
    s_lo = std::min(s_lo, s0);
    s_hi = std::max(s_hi, s0);
    e_lo = std::min(e_lo, e0);
    e_hi = std::max(e_hi, e0);
  }
  const bool wg_ok = nb > 0 && e_hi >= s_lo && e_lo >= s_lo;
  const double cyc = (double)(v[2] - v[0]), ticks = (double)(v[3] - v[1]);  // s_memrealtime: 100 MHz
  const int H = H_of(c);
  auto us = [&](int a, int b) { return v[a] && v[b] && v[b] >= v[a] ? (double)(v[b] - v[a]) / 100.0 : 0.0; };
  const double vals[10] = {ticks > 0 ? cyc * 100.0 / ticks : 0.0,  // shader clock, MHz (ticks: 100 MHz)
                           H > 0 ? cyc / H : 0.0, ticks / 100.0, cyc,
                           us(4, 1),   // workgroup start -> chain start
                           us(3, 5),   // chain end -> every role done
                           us(5, 6),   // -> leaf record written
                           wg_ok ? (double)(s_hi - s_lo) / 100.0 : 0.0,   // first -> last workgroup start
                           wg_ok ? (double)(e_hi - e_lo) / 100.0 : 0.0,   // first -> last record written
                           wg_ok ? (double)(e_hi - s_lo) / 100.0 : 0.0};  // first start -> last record
  for (int i = 0; i < n && i < 10; ++i) out[i] = vals[i];
  // then, per workgroup b, the time from the first workgroup start to b's record (microseconds)
  for (int b = 0; b < nb && 10 + b < n; ++b)
    out[10 + b] = wg_ok ? (double)(v[kClkBase + 2 * b + 1] - s_lo) / 100.0 : 0.0;
  // then (resident server) the stamps of the last 8 steps (kClkServer ring), microseconds from the
  // oldest stamp of the ring (0 = not stamped): out[10 + nb + 8 r + k], r = 0..7 in step order
  uint64_t lo = UINT64_MAX;
  for (int k = 0; k < 64; ++k)
    if (v[kClkServer + k]) lo = std::min(lo, v[kClkServer + k]);
  const int last = (int)(c->sb.seq & 7);
  for (int r = 0; r < 8; ++r)
    for (int k = 0; k < 8; ++k) {
      const int idx = 10 + nb + 8 * r + k;
      const uint64_t x = v[kClkServer + 8 * ((last + 1 + r) & 7) + k];
      if (idx < n) out[idx] = x && lo != UINT64_MAX ? (double)(x - lo) / 100.0 : 0.0;
    }
  return MPPI_OK;
}

int mppi_get_launch_info(mppi_ctx* c, int64_t* info, int32_t n) {
  if (!c || !info) return fail(MPPI_EINVAL, "null argument");
  const Plan& pl = c->last.plan;
  const int64_t v[19] = {0, pl.block, pl.blocks, pl.W, pl.Wr, (int64_t)pl.lds_bytes, c->last.fin_kind,
                         c->last.fin_P, c->last.fin_ncol, c->last.fin_groups, pl.ucache_steps, c->last.resident ? 1 : 0,
                         c->srv.launches, c->srv.steps, c->srv.failed, c->srv.relaunches, c->srv.fallbacks,
                         c->srv.cadence_steps,
                         (c->dem.rinv_res != 0.0f ? 1 : 0) | (c->cmap.rinv_res != 0.0f ? 2 : 0)};
  for (int i = 0; i < n && i < 19; ++i) info[i] = v[i];
  return MPPI_OK;
}

int mppi_sync(mppi_ctx* c) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return MPPI_OK;
}

int mppi_debug_hold(int32_t device, void* stream, int32_t groups, int32_t lds_bytes, int32_t microseconds) {
  if (groups < 1 || groups > 65536 || lds_bytes < 64 || (size_t)lds_bytes > kLdsBytes || microseconds < 0 ||
      microseconds > 1000000)
    return fail(MPPI_EINVAL, "debug_hold: groups in [1, 65536], lds_bytes in [64, 160 KiB], microseconds <= 1e6");
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(launch_hold(groups, (size_t)lds_bytes, (uint64_t)microseconds * 100, (hipStream_t)stream));
  return MPPI_OK;
}

int mppi_selftest(mppi_ctx* c, int32_t what, int64_t n, uint64_t seed, int64_t* mismatches) {
  if (!c || !mismatches) return fail(MPPI_EINVAL, "null argument");
  if (int rc_q = quiesce(c)) return rc_q;
  if (what < 0 || what > 6 || n < 0 || (what == 5 && n > 2 + 0x4C000000LL) || (what == 6 && n > (8193LL << 18)))
    return fail(MPPI_EINVAL, "bad selftest arguments");
  HIP_TRY(hipSetDevice(c->device));
  DeviceBuf<unsigned long long> d;
  HIP_TRY(d.alloc(sizeof(unsigned long long)));
  unsigned long long h = 0;
  hipError_t e = hipMemsetAsync(d, 0, sizeof(unsigned long long), c->stream);
  if (e == hipSuccess) e = launch_selftest(what, n, seed, d, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(&h, d, sizeof(h), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(MPPI_EHIP, std::string("selftest: ") + hipGetErrorString(e));
  *mismatches = (int64_t)h;
  return MPPI_OK;
}

int mppi_rollout_python25d(mppi_ctx* c, int64_t n, int32_t H, const double* x0, const double* y0,
                           const double* heading, const double* lin_vel, const double* ang_vel, double dt,
                           double half_width, double resolution, double bound, double* traj, int32_t* valid) {
  if (!c) return fail(MPPI_EINVAL, "null context");
  if (int rc_q = quiesce(c)) return rc_q;
  if (n < 0 || H < 1) return fail(MPPI_EINVAL, "python25d: need n >= 0 and H >= 1");
  if (n == 0) return MPPI_OK;
  if (!x0 || !y0 || !heading || !lin_vel || !ang_vel || !traj || !valid)
    return fail(MPPI_EINVAL, "python25d: null argument");
  if (!c->dem.Z) return fail(MPPI_ESTATE, "python25d: set a DEM first");
  if (!(resolution > 0.0) || !(half_width > 0.0)) return fail(MPPI_EINVAL, "python25d: bad grid geometry");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const size_t nH = (size_t)n * H;
  const size_t bytes = (5 * (size_t)n + 2 * nH + 3 * nH) * sizeof(double) + (size_t)n * sizeof(int32_t);
  DeviceBuf<char> buf;
  HIP_TRY(buf.alloc(bytes));
  double* d = (double*)buf.get();
  P25Args a;
  a.Z = c->dem.Z;
  a.rows = c->dem.rows;
  a.cols = c->dem.cols;
  a.hw = half_width;
  a.res = resolution;
  a.xstep = (half_width - -half_width) / (double)(c->dem.cols - 1);
  a.ystep = (half_width - -half_width) / (double)(c->dem.rows - 1);
  a.dt = dt;
  a.bound = bound;
  a.n = n;
  a.H = H;
  a.x0 = d;
  a.y0 = d + n;
  a.hd = d + 2 * n;
  a.v = d + 5 * n;
  a.w = a.v + nH;
  a.traj = d + 5 * n + 2 * nH;
  a.valid = (int32_t*)(a.traj + 3 * nH);
  hipError_t e = hipMemcpyAsync((void*)a.x0, x0, n * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)a.y0, y0, n * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)a.hd, heading, 3 * n * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)a.v, lin_vel, nH * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync((void*)a.w, ang_vel, nH * sizeof(double), hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) e = launch_python25d(a, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(traj, a.traj, 3 * nH * sizeof(double), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(valid, a.valid, n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  if (e != hipSuccess) return fail(MPPI_EHIP, std::string("python25d: ") + hipGetErrorString(e));
  return MPPI_OK;
}

}  // extern "C"
