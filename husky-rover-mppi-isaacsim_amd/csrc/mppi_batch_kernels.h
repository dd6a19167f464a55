// Batched closed-loop episodes (mppi_batch_*).  Included by mppi_kernels.hip inside
// namespace mppi: the kernels are built from its device functions (noise_waves, roles_body,
// pair_scale / group_apply, finish_phase2) and compute the bits of the single-context step.
//
// Three plain stream-ordered launches per step (four when the episodes' variants use both
// projections: one rollout launch each), each with a grid dimension for the episode; an
// episode's state lives in its BatchEpisode record (device memory), read with wave-uniform loads
// where a single-context step reads kernel arguments.  No workgroup waits for another or for the
// host (apart from roles_body's own in-workgroup LDS rings).
//
// The task queue (mppi_batch_run_tasks): the finish kernel's campaign form lets the lane whose task
// ended claim the next task of a list in device memory (campaign_claim / campaign_refill); the one
// word two workgroups of a launch share is the list's counter, taken with an agent-scope atomic add.
//
// A scored task list (mppi_batch_set_tasks_scored): the finish kernel's scored form is the campaign form
// whose advance lane also extends the log scorer's critic chains (mppi_score_chain.h) by the row it
// logs, in a per-lane record, and writes the task's score row with its result; the log is optional.
//
// The device-resident step (mppi_batch_step_device): mppi_batch_ingest_kernel writes states held in
// device memory into the records ahead of the noise launch, and the finish kernel's step form hands
// the command and the plan out instead of advancing.  The noise and rollout kernels are the same.
//
// Tracked device steps (mppi_batch_step_tracked): the ingest kernel's tracked form gives the device
// step the notion of a run: it logs the row an ingested state makes, extends the scorer's chains by it
// (the scored form's own device functions), tests the goal and the step cap and writes the run's
// result; the finish kernel's tracked step form keeps the command for the next row.
//
// The wheel forms (mppi_batch_set_wheel_log / _set_score_options): instantiations of the finish and of
// the tracked ingest whose own argument block ends in BatchWheelOpts.  They also log the row's wheel
// contacts beside the row, extend the slope chain over them (score_extend_row_x) and feed the path
// metrics (mppi_path_metrics.h).  The host picks them only when an option is on.
#pragma once

// The normals of every active episode's current step, [blocks][2][H][256] per episode, addressed as
// mppi_noise_kernel addresses them: key = the episode's seed, Philox block step * ((H + 1) / 2) +
// t / 2, global trajectory index.  Grid (G, E), four waves per workgroup; wave w of workgroup g takes
// the wave-units 4 g + w, + 4 G, ... of the episode (noise_waves).
__global__ __launch_bounds__(256) void mppi_batch_noise_kernel(const BatchArgs b, int64_t k_offset) {
  const int e = blockIdx.y;
  const BatchEpisode* ep = b.ep + e;
  if (!ep->active) return;
  const int H = b.H, NB = (H + 1) >> 1;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  float* eps = b.eps + (size_t)e * b.blocks * 2 * H * 256;
  // the leaf blocks the episode runs: no normals for the others (the layout keeps the batch's stride)
  const int blocks = b.scene ? b.scene->rec[e].blocks : b.blocks;
  noise_waves(ep->seed, ep->step * (uint64_t)NB, k_offset, H, (int)blockIdx.x * 4 + wave, blocks * NB * 4,
              (int)gridDim.x * 4, eps, (int)threadIdx.x & 63);
}
// The same under sampling plans (mppi_set_sampling / mppi_batch_set_variant_sampling): the episode's
// plan is the row behind its variant where the caller gave one (antithetic >= 0), else the context's,
// all wave-uniform.  beta > 0 takes the serial form over the episode's (leaf block, 64 trajectories)
// wave-units, the elementwise plans the units above, the default plan the generator above.
__global__ __launch_bounds__(256) void mppi_batch_noise_plan_kernel(const BatchArgs b, int64_t k_offset,
                                                                    const BatchNoisePlan np) {
  const int e = blockIdx.y;
  const BatchEpisode* ep = b.ep + e;
  if (!ep->active) return;
  SamplePlan pl = np.ctx;
  if (np.rows) {
    const int vi = b.ep_var[e];
    if (vi >= 0 && np.rows[vi].antithetic >= 0) pl = np.rows[vi];
  }
  const int H = b.H, NB = (H + 1) >> 1;
  const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
  float* eps = b.eps + (size_t)e * b.blocks * 2 * H * 256;
  const int blocks = b.scene ? b.scene->rec[e].blocks : b.blocks;
  const int q0 = (int)blockIdx.x * 4 + wave, stride = (int)gridDim.x * 4, lane = (int)threadIdx.x & 63;
  if (pl.beta > 0.0f)
    noise_serial(ep->seed, ep->step * (uint64_t)NB, k_offset, H, q0, blocks * 4, stride, eps, lane, pl);
  else if (pl.antithetic | pl.nominal)
    noise_waves<true>(ep->seed, ep->step * (uint64_t)NB, k_offset, H, q0, blocks * NB * 4, stride, eps, lane,
                      pl.antithetic, pl.nominal);
  else
    noise_waves(ep->seed, ep->step * (uint64_t)NB, k_offset, H, q0, blocks * NB * 4, stride, eps, lane);
}

// The role-split rollout of leaf block blockIdx.x of episode blockIdx.y: the launch's RolloutArgs
// (scene and parameters) with the episode's state, derived critic fields, seed, Philox base and
// buffer slices patched in, and, for an episode that holds a variant, its row of the table
// (BatchArgs::var) over the parameters a variant may override.  With a table the launch serves the
// episodes of projection PROJ only (the row's, or the run's for an episode without a variant): a
// workgroup of another projection's episode returns at once, like an inactive one.  With a scene
// table (BatchArgs::scene) the episode's K and, where it holds slots, its DEM, normal table and
// costmap replace the launch's; the grid is the context's, and a leaf block past the episode's
// ceil(K / 256) returns first of all.
// ALT: the critic set is a run-time value, per episode (the row of BatchArgs::crit behind the
// episode's variant, else the launch's); false: no row is set and the context's set is the default,
// and the kernel is the one it was before there was a choice (roles_body's ALT).
template <int PROJ, bool ALT>
__global__ __launch_bounds__(NROLES * 256) void mppi_batch_rollout_kernel(const RolloutArgs a_in, const BatchArgs b) {
  const int e = blockIdx.y;
  // (null: no episode holds a scene slot or a K of its own) a leaf block beyond the episode's K
  if (b.scene && (int)blockIdx.x >= b.scene->rec[e].blocks) return;
  const BatchEpisode* ep = b.ep + e;
  if (!ep->active) return;
  RolloutArgs a = a_in;
  const int H = a.H;
  if (b.scene) {  // patched into the copy: roles_body reads K as kl < a.K only, the scene through a
    const BatchScene s = b.scene->rec[e];
    a.K = s.K;
    if (s.dem >= 0) {
      a.Z = b.scene->dem_z[s.dem];
      a.ntab = b.scene->dem_ntab[s.dem];
    }
    if (s.cm >= 0) a.cm = b.scene->cms[s.cm];
  }
  if (b.var) {  // (null: no episode holds a variant, and the launch is the run's projection)
    const int vi = b.ep_var[e];
    if (vi >= 0) {
      const BatchVariant* v = b.var + vi;
      if (v->proj != PROJ) return;
      a.w_path = v->w_path;
      a.w_slope = v->w_slope;
      a.w_speed = v->w_speed;
      a.w_obs = v->w_obs;
      a.thr = v->thr;
      a.pen = v->pen;
      a.T = v->T;  // leaf_records (its dense / sparse forecast included) reads a.T only
      a.fk = v->fk;
      a.fa = v->fa;
      if constexpr (ALT) {
        if (b.crit) {  // the row's critic set (slope_mode -1: none given, the context's stays)
          const BatchCriticRow cr = b.crit[vi];
          if (cr.slope_mode >= 0) {
            a.slope_body = cr.slope_mode;
            a.w_orient = cr.w_orient;
          }
        }
      }
    } else if (b.proj != PROJ) {
      return;
    }
  }
  a.x0 = ep->x0;
  a.y0 = ep->y0;
  a.h0x = ep->h0x;
  a.h0y = ep->h0y;
  a.h0z = ep->h0z;
  a.wl = ep->wl;
  a.wr = ep->wr;
  a.gx = ep->gx;
  a.gy = ep->gy;
  a.s1 = ep->s1;
  a.s2 = ep->s2;
  a.pf_far = ep->pf_far;
  a.speed_on = ep->speed_on;
  a.igx = ep->igx;
  a.igy = ep->igy;
  a.pf_scale = ep->pf_scale;
  a.seed = ep->seed;
  a.n_base = ep->step * (uint64_t)((H + 1) >> 1);
  a.eps = b.eps + (size_t)e * b.blocks * 2 * H * 256;
  const float* unom = b.unom + ((size_t)e * 2 + ep->cur) * 2 * H;
  a.u_nom1 = unom;
  a.u_nom2 = unom + H;
  a.cost_out = b.cost + (size_t)e * b.k_pad;
  a.nodes = b.nodes + (size_t)e * b.blocks * (2 * H + 2);
  roles_body<256, PROJ, 0, false, false, ALT>(a, (int)blockIdx.x, nullptr);
}

// The goal test (include/mppi.h): inside the tolerance on both axes.  With finite coordinates that is
// !(|dx| > tol || |dy| > tol); a NaN coordinate is never inside, so a pose that is not a number is not
// "reached" (DESIGN.md §4 D13).
__device__ __forceinline__ bool goal_reached(float x, float y, float gx, float gy, float tol) {
  return fabsf(x - gx) <= tol && fabsf(y - gy) <= tol;
}

// The critics' scalar parts of an episode at (x, y) with the goal (gx, gy): state_fields() of
// mppi_capi.cpp, the same float32 operations in the same order (IEEE sqrtf and /).  The one statement
// of the rule on the device: the claim, the advance lane and the ingest all write them through this.
__device__ __forceinline__ void episode_goal_fields(BatchEpisode* ep, float x, float y, float gx, float gy,
                                                    float horizon) {
  const float xd = gx - x;
  const float yd = gy - y;
  const float dist = sqrtf(xd * xd + yd * yd);
  ep->pf_far = dist > horizon ? 1 : 0;
  ep->igx = x + (xd * horizon) / (dist + 1e-6f);
  ep->igy = y + (yd * horizon) / (dist + 1e-6f);
  ep->pf_scale = 1.0f + (2.0f * horizon) / dist;
  ep->speed_on = (dist < 2.0f) ? 0 : 1;
}

// The 11-float state of include/mppi.h's mppi_state (heading as given) between two records that carry its
// names (BatchEpisode, BatchTask, BatchTaskResult), and from the float[11] of an ingest.  Load and store
// alternate field by field, and the ingest's form reads position and goal first, as the copies were written
// before there was one statement of them: the kernels' instruction streams follow that order.
template <class Dst, class Src>
__device__ __forceinline__ void copy_state(Dst& d, const Src& s) {
  d.x0 = s.x0;
  d.y0 = s.y0;
  d.h0x = s.h0x;
  d.h0y = s.h0y;
  d.h0z = s.h0z;
  d.wl = s.wl;
  d.wr = s.wr;
  d.gx = s.gx;
  d.gy = s.gy;
  d.s1 = s.s1;
  d.s2 = s.s2;
}
template <class Dst>
__device__ __forceinline__ void copy_state(Dst& d, const float* s) {
  const float x = s[0], y = s[1], gx = s[7], gy = s[8];
  d.x0 = x;
  d.y0 = y;
  d.h0x = s[2];
  d.h0y = s[3];
  d.h0z = s[4];
  d.wl = s[5];
  d.wr = s[6];
  d.gx = gx;
  d.gy = gy;
  d.s1 = s[9];
  d.s2 = s[10];
}

// The accumulator of a path that starts at (x, y), into a zeroed record: every chain, pending term and count
// stay zero; the goal terms of the start are the critics' scalar parts the episode's record has just received.
__device__ __forceinline__ void score_acc_start(BatchScoreAcc& z, const BatchEpisode* ep, float x, float y) {
  z.x0 = x;
  z.y0 = y;
  z.igx = ep->igx;
  z.igy = ep->igy;
  z.pf_scale = ep->pf_scale;
  z.pf_far = ep->pf_far;
  z.speed_on = ep->speed_on;
}

// One row of a log: the pose, the heading h[0..3) and the command.
__device__ __forceinline__ void log_row(float* lg, float x, float y, float z, const float* h, float v, float w) {
  lg[0] = x;
  lg[1] = y;
  lg[2] = z;
  lg[3] = h[0];
  lg[4] = h[1];
  lg[5] = h[2];
  lg[6] = v;
  lg[7] = w;
}

// The claim rule of the task queue, run by one thread of lane e whose task is over (or that has
// none yet: the first fill).  Takes the next index of the list with one agent-scope atomic add; a
// task whose start already passes the goal test takes no step: its result is written at once
// (steps 0, reached) and the lane claims again.  A claimed task is loaded into the lane: its
// start, the critics' scalar parts by the float32 operations of state_fields() (as the advance
// computes them), seed, Philox step 0, half 0 of the nominal double buffer, no rows, and the lane's
// variant index and scene record, which the next step's kernels read.  With the list exhausted the
// lane goes inactive and leaves the pinned count.  Returns whether a task was loaded (the caller
// then zeroes the lane's nominal double buffer).
// SCORED (a scored list): the lane's accumulator record *acc starts over with the claimed task.
template <bool SCORED>
__device__ __forceinline__ bool campaign_claim(const BatchArgs& b, const BatchCampaign& q, int e, BatchEpisode* ep,
                                               BatchScoreAcc* acc) {
  for (;;) {
    const int i = __hip_atomic_fetch_add(q.next_task, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (i >= q.n) {
      ep->active = 0;
      q.lane[e] = BatchLane{-1, 0, 0};
      __hip_atomic_fetch_add(b.active_count, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return false;
    }
    const BatchTask* t = q.tasks + i;
    const float x = t->x0, y = t->y0, gx = t->gx, gy = t->gy;
    if (goal_reached(x, y, gx, gy, b.goal_tol)) {
      BatchTaskResult* r = q.res + i;
      copy_state(*r, *t);
      r->steps = 0;
      r->reached = 1;
      r->flags = 3;
      continue;
    }
    copy_state(*ep, *t);
    episode_goal_fields(ep, x, y, gx, gy, b.horizon);
    if constexpr (SCORED) {
      BatchScoreAcc z{};
      score_acc_start(z, ep, x, y);
      *acc = z;
    }
    ep->active = 1;
    ep->cur = 0;
    ep->seed = t->seed;
    ep->step = 0;
    ep->steps_run = 0;
    ep->reached = 0;
    q.lane[e] = BatchLane{i, t->max_steps, t->log_base};
    q.ep_var[e] = t->variant;
    q.rec[e] = t->scene;
    q.res[i].flags = 1;
    return true;
  }
}

// The whole workgroup of lane e (nthreads threads, `got`: one int of LDS): thread 0 claims when
// the lane's task is `ended` (its own knowledge; the others pass anything), the decision goes
// through LDS, and on a new task every thread zeroes its share of both halves of the lane's nominal
// double buffer (what mppi_batch_set_episode does with a memset).  Every thread of the workgroup
// calls this: the branch is uniform, the barrier is not inside it.
template <class Form>
__device__ __forceinline__ void campaign_refill(const BatchArgs& b, const Form& form, int e, BatchEpisode* ep,
                                                bool ended, int tid, int nthreads, int* got) {
  BatchScoreAcc* acc = nullptr;  // a scored form: the lane's record
  if constexpr (Form::kScored) acc = form.scored().acc + e;
  if (tid == 0) *got = (ended && campaign_claim<Form::kScored>(b, form.queue(), e, ep, acc)) ? 1 : 0;
  __syncthreads();
  if (*got) {
    float* u = b.unom + (size_t)e * 4 * b.H;
    for (int j = tid; j < 4 * b.H; j += nthreads) u[j] = 0.0f;
  }
}

// One workgroup per episode: the binary tree over its leaf records (tree_reduce of the oracle: the
// count padded to a power of two with empty records; one aligned group of 16 with the empty members
// passing their partners through, as the last pass of mppi_finish_kernel), the mode-2 phase 2 (u_opt
// into the other half of the nominal double buffer, the filtered v / w, row 0 of the optimal
// rollout), then one lane advances the episode by the closed loop's rule (MPPI_Controller.run,
// MPPI_isaac.py:769-784; mppi_amd/batch.py advance_state is the same arithmetic on the host).
//
// CAMPAIGN (mppi_batch_run_tasks): the episode is a lane working through the task list `q`.  Its
// row goes to its task's rows of the log arena, and when the task ends (goal test passed, or the
// row count reaches the task's cap) the advance lane writes the task's result and the workgroup
// refills the lane (campaign_refill above) instead of going inactive.
//
// STEP (mppi_batch_step_device): the plant is the caller's.  Instead of the advance one lane writes
// the command (v, w) to io.cmd[e], flips the nominal double buffer and counts the step, and the
// workgroup copies the 4H + 12 outputs to io.plan[e]: no advance rule, no goal test, no log row, no
// touch of the active count.  The state stays what the ingest kernel (below) wrote.
//
// SCORED (a list set by mppi_batch_set_tasks_scored): the campaign form whose advance lane also
// extends the four critic chains of the log scorer by the row in hand (mppi_score_chain.h: the same
// device functions, the same order in t) and the float64 path length, in the lane's BatchScoreAcc,
// and writes the task's BatchTaskScore with its result.  Two terms wait for the next row, because the
// scorer admits them only when that row exists: the near path term of row t (the sum runs over
// t < L - 1) and the slope term of even row s (it needs row s + 1).  The record is loaded at the head,
// beside lane_steps; only this lane reads or writes it.  With q.log null (keep_log = 0) no row is
// written: a uniform branch around the eight stores.
//
// TRACKED (mppi_batch_step_tracked): the step form with one more store pair: (v, w) into the
// episode's tracking record, where the next tracked ingest finds the command its row is paired with.
//
// The kernel's third argument is the form (mppi_kernels.h): it names which of the above it is and
// hands out the queue, the scored block, the io block, the tracking records and the wheel options.

// Row `row` of a path enters the accumulator: (x, y, z) and v, what the log row holds; (gx, gy) the
// path's goal, cm its costmap.  The one statement of the rule for the scored campaign's advance lane
// and the tracked ingest; cm (cm_size squared cells) is the context's costmap or the one of the path's slot.
// WX (the wheel forms), wheels: the slope chain reads the row's wheel contacts cw (left | right) in place of
// the body waypoint: slope_one on both wheels against the previous even contacts in wa, the larger value
// (the scorer's WHEELS slope wave; critics_warp.py:168-218), in the same order over the even rows.  (wa and
// cw go in by reference and the choice as a flag: behind a pointer that may be null they stayed in memory.)
template <bool WX>
__device__ __forceinline__ void score_extend_row_x(BatchScoreAcc& sa, const BatchYardstick& yd, const float* cm,
                                                   int cm_size, int row, float x, float y, float z, float v, float gx,
                                                   float gy, bool wheels, BatchWheelAcc& wa, const float (&cw)[6]) {
  if (!sa.pf_far) {  // the near branch: the term of row - 1 enters now that this row exists
    if (row >= 1) sa.path = sa.path + sa.path_pend;
    sa.path_pend = chain::path_near(x, y, gx, gy);
  }
  if (WX && wheels) {
    if ((row & 1) == 0) {
      const float l3[3] = {cw[0], cw[1], cw[2]}, r3[3] = {cw[3], cw[4], cw[5]};
      if (row >= 2) {
        const float ls = chain::slope_one(wa.pl, l3), rs = chain::slope_one(wa.pr, r3);
        sa.slope_pend = (ls > rs) ? ls : rs;
      }
#pragma unroll
      for (int i = 0; i < 3; ++i) {
        wa.pl[i] = l3[i];
        wa.pr[i] = r3[i];
      }
    } else if (row >= 3) {
      sa.slope = sa.slope + sa.slope_pend;
    }
  } else if ((row & 1) == 0) {  // an even row s: its term (rows s - 2 and s) waits for row s + 1
    const float c3[3] = {x, y, z};
    if (row >= 2) sa.slope_pend = chain::slope_one(sa.pe, c3);
    sa.pe[0] = x;
    sa.pe[1] = y;
    sa.pe[2] = z;
  } else if (row >= 3) {
    sa.slope = sa.slope + sa.slope_pend;
  }
  if (sa.speed_on) sa.speed = chain::speed(sa.speed, yd.vmax, v);
  const float c = cm[chain::cm_index(yd.hw, yd.res_c, cm_size, x, y)];
  const chain::ObstacleAcc oa = chain::obstacle(sa.obs, sa.col, c, yd.thr, yd.pen);
  sa.obs = oa.acc;
  sa.col = oa.col;
  if (row % 5 == 0) {  // compute_length: the sampled rows 0, 5, 10, ..., float64, no contraction
    if (row > 0) {
      const double dx = (double)x - (double)sa.sx, dy = (double)y - (double)sa.sy, dz = (double)z - (double)sa.sz;
      sa.length = sa.length + __builtin_sqrt((dx * dx + dy * dy) + dz * dz);
    }
    sa.sx = x;
    sa.sy = y;
    sa.sz = z;
  }
}
__device__ __forceinline__ void score_extend_row(BatchScoreAcc& sa, const BatchYardstick& yd, const float* cm,
                                                 int cm_size, int row, float x, float y, float z, float v, float gx,
                                                 float gy) {
  BatchWheelAcc none{};
  const float no_contacts[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  score_extend_row_x<false>(sa, yd, cm, cm_size, row, x, y, z, v, gx, gy, false, none, no_contacts);
}

// The score row of a path that ended with row `row` at (x, y), into table[index]: L = row + 1 rows; the
// far branch and the orientation critic read the last ones (sa.lx, sa.ly: row - 1).
template <class Index>
__device__ __forceinline__ void score_write(BatchTaskScore* table, Index index, const BatchScoreAcc& sa,
                                            const BatchYardstick& yd, int row, float x, float y, float gx, float gy) {
  const float pf = sa.pf_far ? chain::path_far(x, y, sa.igx, sa.igy, sa.pf_scale) : sa.path;
  const float po = row >= 1 ? chain::orientation(gx, gy, sa.x0, sa.y0, sa.lx, sa.ly, x, y) : 0.0f;
  BatchTaskScore* o = table + index;
  o->cost = chain::combine(yd.w_path, yd.w_slope, yd.w_speed, yd.w_obs, yd.w_orient, pf, sa.slope, sa.speed, sa.obs,
                           po);
  o->terms[0] = pf;
  o->terms[1] = sa.slope;
  o->terms[2] = sa.speed;
  o->terms[3] = sa.obs;
  o->collisions = sa.col;
  o->rows = row + 1;
  o->length = sa.length;
}

template <class Form>
__global__ __launch_bounds__(FIN_THREADS) void mppi_batch_finish_kernel(const FinishArgs f_in, const BatchArgs b,
                                                                         const Form form) {
  // WX: a wheel form (mppi_batch_set_wheel_log / _set_score_options): the advance lane also reads row 0 of
  // the optimal rollout's wheel contacts (floats 4H + 6 .. 4H + 11 of the finish output), logs them beside
  // the row, extends the slope chain in its wheel form and the path metrics by them
  constexpr bool WX = Form::kWheels, SCORED = Form::kScored, CAMPAIGN = Form::kCampaign, TRACKED = Form::kTracked,
                 STEP = Form::kStep;
  static_assert((!SCORED || CAMPAIGN) && (!TRACKED || STEP) && !(CAMPAIGN && STEP) && !(WX && STEP),
                "a scored form is a campaign, a tracked form a step; a step neither runs a queue nor logs wheels");
  const BatchCampaign* q = nullptr;
  const BatchScoredCampaign* sc = nullptr;
  const BatchWheelOpts* wx = nullptr;
  if constexpr (CAMPAIGN) q = &form.queue();
  if constexpr (SCORED) sc = &form.scored();
  if constexpr (WX) wx = &form.wheels();
  extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
  const int e = blockIdx.x;
  BatchEpisode* ep = b.ep + e;
  if (!ep->active) return;
  const int tid = threadIdx.x;
  BatchLane ln{};
  int lane_steps = 0;  // CAMPAIGN: loaded here, off the advance lane's serial path
  if constexpr (CAMPAIGN) {
    ln = q->lane[e];
    lane_steps = q->lane_steps[e];
  }
  BatchScoreAcc sa{};         // SCORED: the lane's chains so far, loaded here as lane_steps is
  const float* cm = nullptr;  // SCORED: the task's costmap
  if constexpr (SCORED) {
    sa = sc->acc[e];
    cm = sc->cm;
  }
  BatchWheelAcc wa{};   // WX, SCORED: the lane's previous even contacts and its metrics state, loaded here too
  PathMetricsAcc ma{};
  if constexpr (WX && SCORED) {
    if (wx->wacc) wa = wx->wacc[e];
    if (wx->macc) ma = wx->macc[e];
  }
  FinishArgs f = f_in;
  const int H = f.H, E = 2 * H + 2;
  float sigma_base = b.sigma_base, sigma_div = b.sigma_div;
  if (b.var) {
    const int vi = b.ep_var[e];
    if (vi >= 0) {
      const BatchVariant* v = b.var + vi;
      f.T = v->T;
      f.ok = v->ok;
      f.oa = v->oa;
      sigma_base = v->sigma_base;
      sigma_div = v->sigma_div;
    }
  }
  int n = b.blocks;  // the episode's leaf records
  if (b.scene) {
    const BatchScene s = b.scene->rec[e];
    n = s.blocks;
    if (s.dem >= 0) {  // row 0 of the optimal rollout reads the DEM
      f.Z = b.scene->dem_z[s.dem];
      f.ntab = b.scene->dem_ntab[s.dem];
    }
    if constexpr (SCORED) {
      if (s.cm >= 0) cm = b.scene->cms[s.cm];
    }
  }
  const int cur_buf = ep->cur;
  const float gx = ep->gx, gy = ep->gy;
  const int row = ep->steps_run;
  f.mode = 2;
  f.done = nullptr;
  f.x0 = ep->x0;
  f.y0 = ep->y0;
  f.h0x = ep->h0x;
  f.h0y = ep->h0y;
  f.h0z = ep->h0z;
  f.wl = ep->wl;
  f.wr = ep->wr;
  f.u_nom_next = b.unom + ((size_t)e * 2 + (cur_buf ^ 1)) * 2 * H;
  f.out = b.fin + (size_t)e * (7 * H + 12);
  f.tail_in = f.out + 4 * H + 12;
  // ---------------- (1) tree: the n <= 16 records -> root in lnode[0..E)
  double* lnode = reinterpret_cast<double*>(smem_raw);
  PairScale* lps = reinterpret_cast<PairScale*>(smem_raw + (size_t)E * sizeof(double));
  const double* recs = b.nodes + (size_t)e * b.blocks * E;
  if (n > 1) {
    float* lm = reinterpret_cast<float*>(lps + 15);
    if (tid < 16) lm[tid] = (tid < n) ? (float)recs[(size_t)tid * E] : INFINITY;
    __syncthreads();
    int base = 0;
#pragma unroll
    for (int w = 8; w >= 1; w >>= 1) {
      PairScale p;
      if (tid < w) {
        p = pair_scale(lm[2 * tid], lm[2 * tid + 1], f.T);
        lps[base + tid] = p;
      }
      __syncthreads();
      if (tid < w) lm[tid] = p.m;
      __syncthreads();
      base += w;
    }
    for (int j = tid; j < E; j += FIN_THREADS) {
      double v[16];
#pragma unroll
      for (int i = 0; i < 16; ++i) v[i] = recs[(size_t)min(i, n - 1) * E + j];
      lnode[j] = group_apply<16>(lps, v, j);
    }
  } else {
    for (int j = tid; j < E; j += FIN_THREADS) lnode[j] = recs[j];
  }
  __syncthreads();
  // ---------------- (2) u_opt = V / S (zero when no trajectory has a finite cost) and phase 2
  const double S = lnode[1];
  const float ures = (tid < 2 * H && S > 0.0) ? (float)(lnode[2 + tid] / S) : 0.0f;
  __syncthreads();  // lnode is dead from here on
  finish_phase2(f, ures, smem_raw, tid, FIN_THREADS);
  if constexpr (STEP) {
    // ---------------- (3') the command and the plan out (after finish_phase2's closing barrier; its
    // outputs were written through, so agent-scope loads see them)
    const BatchIo* io = &form.io();
    auto ld = [&](int i) __attribute__((always_inline)) {
      return __hip_atomic_load(f.out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const int nplan = 4 * H + 12;
    if (io->plan) {
      float* plan = io->plan + (size_t)e * nplan;
      for (int j = tid; j < nplan; j += FIN_THREADS) plan[j] = ld(j);
    }
    if (tid == 0) {
      if (io->cmd) {
        io->cmd[2 * (size_t)e] = ld(2 * H);
        io->cmd[2 * (size_t)e + 1] = ld(3 * H);
      }
      if constexpr (TRACKED) {  // the command the episode's next row is paired with
        BatchTrackRec* tr = form.track() + e;
        tr->v = ld(2 * H);
        tr->w = ld(3 * H);
      }
      ep->cur = cur_buf ^ 1;
      ep->step = ep->step + 1;
    }
    return;
  }
  // ---------------- (3) advance (finish_phase2 ends with every output store complete and a barrier;
  // the outputs were written through, so agent-scope loads see them)
  if constexpr (!CAMPAIGN) {
    if (tid != 0) return;
  }
  bool ended = false;  // CAMPAIGN, advance lane: the task is over
  if (!CAMPAIGN || tid == 0) {
    auto ld = [&](int i) __attribute__((always_inline)) {
      return __hip_atomic_load(f.out + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    };
    const float v = ld(2 * H), w = ld(3 * H);
    const float x = ld(4 * H), y = ld(4 * H + 1), z = ld(4 * H + 2);
    // heading: row 0 widened to float64 and divided by its norm ((a a + b b) + c c, no fma), each
    // component rounded to float32 (robot.heading_vector / np.linalg.norm, MPPI_isaac.py:493)
    const double d0 = (double)ld(4 * H + 3), d1 = (double)ld(4 * H + 4), d2 = (double)ld(4 * H + 5);
    const double nn = __builtin_sqrt((d0 * d0 + d1 * d1) + d2 * d2);
    const float hx = (float)(d0 / nn), hy = (float)(d1 / nn), hz = (float)(d2 / nn);
    bool logs = row < (CAMPAIGN ? ln.max_steps : b.log_cap);
    if constexpr (SCORED) logs = logs && q->log != nullptr;
    float cw[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};  // WX: left_wheel_sim[0] | right_wheel_sim[0]
    if constexpr (WX) {
#pragma unroll
      for (int i = 0; i < 6; ++i) cw[i] = ld(4 * H + 6 + i);
      if (logs && wx->wlog) {  // the row of the same index in the parallel array
        float* wl = wx->wlog + (CAMPAIGN ? (size_t)ln.log_base + row : (size_t)e * b.log_cap + row) * 6;
#pragma unroll
        for (int i = 0; i < 6; ++i) wl[i] = cw[i];
      }
    }
    if (logs) {
      const float h[3] = {hx, hy, hz};
      log_row(CAMPAIGN ? q->log + ((size_t)ln.log_base + row) * 8 : b.log + ((size_t)e * b.log_cap + row) * 8, x, y, z,
              h, v, w);
    }
    const float ww = (w * w) / sigma_div;
    const float half = (w * b.rwheel) / 2.0f;
    ep->x0 = x;
    ep->y0 = y;
    ep->h0x = hx;
    ep->h0y = hy;
    ep->h0z = hz;
    ep->wl = v - half;
    ep->wr = v + half;
    ep->s1 = fmaxf(sigma_base, sigma_base - ww);
    ep->s2 = fmaxf(sigma_base, sigma_base + ww);
    episode_goal_fields(ep, x, y, gx, gy, b.horizon);
    ep->cur = cur_buf ^ 1;
    ep->step = ep->step + 1;
    ep->steps_run = row + 1;
    const bool reached = goal_reached(x, y, gx, gy, b.goal_tol);
    // row `row` of the task's path enters the chains: (x, y, z) and v, what the log row holds
    if constexpr (SCORED && WX) {
      score_extend_row_x<true>(sa, sc->y, cm, sc->cm_size, row, x, y, z, v, gx, gy, wx->wacc != nullptr, wa, cw);
      if (wx->macc) metrics_row(ma, row, x, y, z);
    } else if constexpr (SCORED) {
      score_extend_row(sa, sc->y, cm, sc->cm_size, row, x, y, z, v, gx, gy);
    }
    if constexpr (CAMPAIGN) {
      q->lane_steps[e] = lane_steps + 1;
      ended = reached || row + 1 >= ln.max_steps;
      if (ended) {
        BatchTaskResult* r = q->res + ln.task;
        // (the state the episode has just received and its goal, from the values in hand: a record built
        // for copy_state, or a read back from *ep, changes the kernel's instruction stream)
        r->x0 = x;
        r->y0 = y;
        r->h0x = hx;
        r->h0y = hy;
        r->h0z = hz;
        r->wl = v - half;
        r->wr = v + half;
        r->gx = gx;
        r->gy = gy;
        r->s1 = fmaxf(sigma_base, sigma_base - ww);
        r->s2 = fmaxf(sigma_base, sigma_base + ww);
        r->steps = row + 1;
        r->reached = reached ? 1 : 0;
        r->flags = 3;
      }
      if constexpr (SCORED) {
        if (ended) {
          score_write(sc->score, ln.task, sa, sc->y, row, x, y, gx, gy);
          if constexpr (WX)
            if (wx->macc) wx->metrics[ln.task] = ma.m;
        } else {  // (the claim resets the record of a lane whose task ended)
          sa.lx = x;
          sa.ly = y;
          sc->acc[e] = sa;
          if constexpr (WX) {  // (row 0 of the next task starts both over)
            if (wx->wacc) wx->wacc[e] = wa;
            if (wx->macc) wx->macc[e] = ma;
          }
        }
      }
    } else if (reached) {
      ep->active = 0;
      ep->reached = 1;
      __hip_atomic_fetch_add(b.active_count, -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
  }
  if constexpr (CAMPAIGN) campaign_refill(b, form, e, ep, ended, tid, FIN_THREADS, reinterpret_cast<int*>(smem_raw));
}

// The first fill of a campaign: every lane claims as a finishing lane does (a scored list's claim also
// resets the lane's accumulator record).  Grid E, one wave each.
template <class Form>
__global__ __launch_bounds__(64) void mppi_batch_claim_kernel(const BatchArgs b, const Form form) {
  __shared__ int got;
  const int e = blockIdx.x;
  campaign_refill(b, form, e, b.ep + e, true, (int)threadIdx.x, 64, &got);
}

// The way into the episode record for a plant that lives on the device (mppi_batch_step_device):
// episode e takes this step iff it is set (is_set[e], the host's flag mirrored in device memory) and
// io.mask lets it; its record then takes the state of io.states[e] (11 floats in mppi_state order,
// the heading as given) and the critics' scalar parts of that state, and `reached` is cleared (no
// goal test has seen the new state).  On a reset the workgroup zeroes both halves of the nominal
// double buffer and the lane restarts the step index, the buffer half and, where given, the seed.
// An episode that does not step keeps its whole record but `active`, which every launch of the
// step reads.  Grid E, one wave each; e is the workgroup's, so every read is wave-uniform.  No LDS, no
// waits: the noise and rollout kernels read the record behind the kernel boundary.
__device__ __forceinline__ void plain_ingest(const BatchArgs& b, const BatchIo& io, const int* is_set) {
  const int e = blockIdx.x;
  BatchEpisode* ep = b.ep + e;
  const bool on = is_set[e] != 0 && (!io.mask || io.mask[e] != 0);
  const bool reset = on && io.reset && io.reset[e] != 0;
  if (threadIdx.x == 0) {
    ep->active = on ? 1 : 0;
    if (on) {
      const float* s = io.states + (size_t)e * 11;
      const float x = s[0], y = s[1], gx = s[7], gy = s[8];
      copy_state(*ep, s);
      episode_goal_fields(ep, x, y, gx, gy, b.horizon);
      ep->reached = 0;
      if (reset) {
        ep->cur = 0;
        ep->step = 0;
        if (io.seeds) ep->seed = io.seeds[e];
      }
    }
  }
  if (reset) {
    float* u = b.unom + (size_t)e * 4 * b.H;
    for (int j = (int)threadIdx.x; j < 4 * b.H; j += 64) u[j] = 0.0f;
  }
}

// The result row of a run that ended: the state of the ending ingest (11 floats in mppi_state order),
// its rows, the goal test's answer and the status.  The score row is the caller's.
// (Field by field in the record's order: s is device memory that the kernel has written around, and the
// ingests' copy_state, which reads position and goal first, gives the tracked ingests another stream.)
__device__ __forceinline__ void run_result(BatchTaskResult* r, const float* s, int steps, int reached, int status) {
  r->x0 = s[0];
  r->y0 = s[1];
  r->h0x = s[2];
  r->h0y = s[3];
  r->h0z = s[4];
  r->wl = s[5];
  r->wr = s[6];
  r->gx = s[7];
  r->gy = s[8];
  r->s1 = s[9];
  r->s2 = s[10];
  r->steps = steps;
  r->reached = reached;
  r->flags = status;
}

// The tracked form of the ingest (mppi_batch_step_tracked): the plain form's rule for which episode
// takes the step and what its record receives, and around it the run.  Lane 0, in this order:
//   a reset that finds an unfinished run with rows writes that run's result (abandoned: the state
//   and the last row are the record's, which the previous ingest wrote) and begins a new run;
//   the state that begins a run (a reset, or the first ingest after mppi_batch_set_episode) is its
//   start: the accumulator starts over with the goal terms of that state, no row; a start inside the
//   tolerance ends the run at once (steps 0, reached, a score row of zeros);
//   any other ingested state is row rows: (x, y, z, the heading as given, v, w) with (v, w) the
//   command the previous step left in the record and z the caller's, or the height of the episode's
//   DEM at (x, y) by the rollout's own lookup (Dem::corners and bilinear, IEEE division); the row goes
//   to the log (keep_log), into the chains (score_extend_row), then the goal test on the ingested
//   state and the cap decide whether the run ends: the result and the score row (score_write) go to
//   slot e * runs_per_episode + (the episode's run count) if there is one, and the count grows.
// An ended episode is inactive for the step's other launches until its next reset, and keeps its
// record, nominal sequence and step index.  done[e] reads the status of every set episode (0 for one
// never set, so the whole array is written at every step).  The slot
// depends on (e, run count) only: no atomic, and the active count is not touched.  One costmap gather
// per row, and four DEM loads when z is null; no LDS, no waits.
//
// WX (the BatchWheelTrack form; mppi_batch_set_wheel_log / _set_score_options
// before tracking was set): the row also gets its wheel contacts, formed from the ingested pose by the
// rollout's own rule (wheel_contacts below) on the episode's DEM; they go to the wheel log beside the row,
// into the slope chain's wheel form and, with (x, y, z), into the path metrics, whose row is written
// beside the run's score row.
//
// The contacts of a pose (projection_warp.py:331-347; oracle/mppi_ref.py rollout3d :306-315 with `cur`
// the row's heading as given): q = the corners of the cell of (x, y), n = normal_on_grid(q),
// c = cross(n, heading), r = (off c.x, off c.y), left = (x + r.x, y + r.y, Z[cell]), right the same with
// -r; truncating cell index with clamping, IEEE / and sqrtf (Dem's <false> forms).
__device__ __forceinline__ void wheel_contacts(const Dem& d, float x, float y, float hx, float hy, float hz, float off,
                                               float (&cw)[6]) {
  bool unused = false;
  float q[4];
  d.corners<false>(x, y, q, unused);
  const float hr = (-d.res) / 2.0f;
  const float vx = hr * (((q[1] - q[0]) - q[2]) + q[3]);
  const float vy = hr * (((q[2] - q[0]) - q[1]) + q[3]);
  const float vz = d.res * d.res;
  const float norm = sqrtf((vx * vx + vy * vy) + vz * vz);
  const float nx = vx / norm, ny = vy / norm, nz = vz / norm;
  const float rx = off * (ny * hz - nz * hy);
  const float ry = off * (nz * hx - nx * hz);
  int i, j;
  cw[0] = x + rx;
  cw[1] = y + ry;
  d.cell<false>(cw[0], cw[1], i, j, unused);
  cw[2] = d.at(j, i);
  cw[3] = x - rx;
  cw[4] = y - ry;
  d.cell<false>(cw[3], cw[4], i, j, unused);
  cw[5] = d.at(j, i);
}

template <bool WX>
__device__ __forceinline__ void tracked_ingest(const BatchArgs& b, const BatchIo& io, const int* __restrict__ is_set,
                                               const BatchTrack& t, const BatchWheelOpts* wx) {
  const int e = blockIdx.x;
  BatchEpisode* ep = b.ep + e;
  const bool set = is_set[e] != 0;
  const bool on = set && (!io.mask || io.mask[e] != 0);
  const bool reset = on && io.reset && io.reset[e] != 0;
  if (threadIdx.x == 0) {
    BatchTrackRec* tr = t.rec + e;
    int ended = tr->ended;
    if (on && (reset || !ended)) {
      BatchTrackRec r = *tr;
      int runs = t.runs[e];
      const float* cm = t.cm;
      const float* Z = t.Z;
      if (b.scene) {
        const BatchScene sl = b.scene->rec[e];
        if (sl.cm >= 0) cm = b.scene->cms[sl.cm];
        if (sl.dem >= 0) Z = b.scene->dem_z[sl.dem];
      }
      if (reset && !r.ended && !r.fresh && r.rows >= 1) {  // abandoned
        if (runs < t.runs_per_episode) {
          BatchRunResult* o = t.results + (size_t)e * t.runs_per_episode + runs;
          const float last[11] = {ep->x0, ep->y0, ep->h0x, ep->h0y, ep->h0z, ep->wl, ep->wr, ep->gx, ep->gy, ep->s1, ep->s2};
          run_result(&o->r, last, r.rows, 0, kRunAbandoned);
          r.acc.lx = r.px;
          r.acc.ly = r.py;
          score_write(&o->s, 0, r.acc, t.y, r.rows - 1, last[0], last[1], r.gx, r.gy);
          if constexpr (WX)
            if (wx->macc) wx->metrics[(size_t)e * t.runs_per_episode + runs] = wx->macc[e].m;
        }
        ++runs;
      }
      const float* s = io.states + (size_t)e * 11;
      const float x = s[0], y = s[1], gx = s[7], gy = s[8];
      copy_state(*ep, s);
      episode_goal_fields(ep, x, y, gx, gy, b.horizon);
      if (reset) {
        ep->cur = 0;
        ep->step = 0;
        if (io.seeds) ep->seed = io.seeds[e];
      }
      const bool reached = goal_reached(x, y, gx, gy, b.goal_tol);
      BatchRunResult* o = runs < t.runs_per_episode ? t.results + (size_t)e * t.runs_per_episode + runs : nullptr;
      if (reset || r.fresh) {  // the run's start
        BatchTrackRec z{};
        score_acc_start(z.acc, ep, x, y);
        z.gx = gx;
        z.gy = gy;
        r = z;
        if (t.keep_log) ep->steps_run = 0;
        if (reached) {
          if (o) {
            run_result(&o->r, s, 0, 1, kRunReached);
            o->s = BatchTaskScore{};
            if constexpr (WX)
              if (wx->macc) wx->metrics[(size_t)e * t.runs_per_episode + runs] = PathMetrics{0.0, 0.0, 0.0, 0.0};
          }
          ++runs;
          r.ended = kRunReached;
        }
      } else {  // row r.rows of the run
        const int row = r.rows;
        float z;
        if (t.z) {
          z = t.z[e];
        } else {
          Dem d;
          d.init(Z, t.rows, t.grid, t.x_min, t.y_min, t.res);
          bool unused = false;
          float q[4];
          d.corners<false>(x, y, q, unused);
          z = bilinear<false>(x, y, q, d.rr<false>(), unused);
        }
        if (t.keep_log) {
          if (row < b.log_cap) log_row(b.log + ((size_t)e * b.log_cap + row) * 8, x, y, z, s + 2, r.v, r.w);
          ep->steps_run = min(row + 1, b.log_cap);
        }
        if constexpr (WX) {
          float cw[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
          const bool log_w = wx->wlog && t.keep_log && row < b.log_cap;
          if (log_w || wx->wacc) {
            Dem d;
            d.init(Z, t.rows, t.grid, t.x_min, t.y_min, t.res);
            wheel_contacts(d, x, y, s[2], s[3], s[4], wx->off, cw);
          }
          if (log_w) {
            float* wl = wx->wlog + ((size_t)e * b.log_cap + row) * 6;
#pragma unroll
            for (int i = 0; i < 6; ++i) wl[i] = cw[i];
          }
          BatchWheelAcc wa{};
          if (wx->wacc) wa = wx->wacc[e];
          score_extend_row_x<true>(r.acc, t.y, cm, t.cm_size, row, x, y, z, r.v, r.gx, r.gy, wx->wacc != nullptr, wa, cw);
          if (wx->wacc) wx->wacc[e] = wa;
          if (wx->macc) {
            PathMetricsAcc ma = wx->macc[e];
            metrics_row(ma, row, x, y, z);
            wx->macc[e] = ma;
          }
        } else {
          score_extend_row(r.acc, t.y, cm, t.cm_size, row, x, y, z, r.v, r.gx, r.gy);
        }
        r.rows = row + 1;
        if (reached || row + 1 >= t.max_steps) {
          if (o) {
            run_result(&o->r, s, row + 1, reached ? 1 : 0, reached ? kRunReached : kRunCap);
            score_write(&o->s, 0, r.acc, t.y, row, x, y, r.gx, r.gy);
            if constexpr (WX)
              if (wx->macc) wx->metrics[(size_t)e * t.runs_per_episode + runs] = wx->macc[e].m;
          }
          ++runs;
          r.ended = reached ? kRunReached : kRunCap;
        } else {
          r.px = r.acc.lx;
          r.py = r.acc.ly;
          r.acc.lx = x;
          r.acc.ly = y;
        }
      }
      ep->reached = r.ended == kRunReached ? 1 : 0;
      *tr = r;
      t.runs[e] = runs;
      ended = r.ended;
    }
    ep->active = (on && !ended) ? 1 : 0;
    if (t.done) t.done[e] = set ? ended : 0;
  }
  if (reset) {
    float* u = b.unom + (size_t)e * 4 * b.H;
    for (int j = (int)threadIdx.x; j < 4 * b.H; j += 64) u[j] = 0.0f;
  }
}

// The ingest of the form: plain, tracked, or tracked with the wheel options.
template <class Form>
__global__ __launch_bounds__(64) void mppi_batch_ingest_kernel(const BatchArgs b, const BatchIo io,
                                                                const int* __restrict__ is_set, const Form form) {
  if constexpr (!Form::kTracked) plain_ingest(b, io, is_set);
  else if constexpr (Form::kWheels) tracked_ingest<true>(b, io, is_set, form.track(), &form.wheels());
  else tracked_ingest<false>(b, io, is_set, form.track(), nullptr);
}

hipError_t launch_batch_noise(const BatchArgs& b, int64_t k_offset, hipStream_t st, const BatchNoisePlan& np) {
  // about four wave-units (two noise_waves iterations) per wave
  const int units = b.blocks * ((b.H + 1) >> 1) * 4;
  const unsigned g = (unsigned)std::min(std::max((units + 15) / 16, 1), 64);
  // (no plan row and the default plan on the context: the kernel as it was before there were plans)
  const bool plain = !np.rows && !np.ctx.antithetic && !np.ctx.nominal && !(np.ctx.beta > 0.0f);
  if (plain) hipLaunchKernelGGL(mppi_batch_noise_kernel, dim3(g, (unsigned)b.E), dim3(256), 0, st, b, k_offset);
  else hipLaunchKernelGGL(mppi_batch_noise_plan_kernel, dim3(g, (unsigned)b.E), dim3(256), 0, st, b, k_offset, np);
  return hipGetLastError();
}

hipError_t launch_batch_rollout(const RolloutArgs& a, const BatchArgs& b, size_t lds, hipStream_t st, int proj) {
  const dim3 g((unsigned)b.blocks, (unsigned)b.E), t(NROLES * 256);
  // (a batch with no critic row on a context with the default set runs the form compiled without the choice)
  const bool alt = b.crit != nullptr || a.slope_body || a.w_orient != 0.0f;
  if (proj == 3) {
    if (alt) hipLaunchKernelGGL((mppi_batch_rollout_kernel<3, true>), g, t, lds, st, a, b);
    else hipLaunchKernelGGL((mppi_batch_rollout_kernel<3, false>), g, t, lds, st, a, b);
  } else {
    if (alt) hipLaunchKernelGGL((mppi_batch_rollout_kernel<2, true>), g, t, lds, st, a, b);
    else hipLaunchKernelGGL((mppi_batch_rollout_kernel<2, false>), g, t, lds, st, a, b);
  }
  return hipGetLastError();
}

template <class Form>
hipError_t launch_batch_finish(const FinishArgs& f, const BatchArgs& b, const Form& form, size_t lds, hipStream_t st) {
  hipLaunchKernelGGL(mppi_batch_finish_kernel<Form>, dim3((unsigned)b.E), dim3(FIN_THREADS), lds, st, f, b, form);
  return hipGetLastError();
}
template <class Form>
hipError_t launch_batch_ingest(const BatchArgs& b, const BatchIo& io, const int* is_set, const Form& form,
                               hipStream_t st) {
  hipLaunchKernelGGL(mppi_batch_ingest_kernel<Form>, dim3((unsigned)b.E), dim3(64), 0, st, b, io, is_set, form);
  return hipGetLastError();
}
template <class Form>
hipError_t launch_batch_claim(const BatchArgs& b, const Form& form, hipStream_t st) {
  hipLaunchKernelGGL(mppi_batch_claim_kernel<Form>, dim3((unsigned)b.E), dim3(64), 0, st, b, form);
  return hipGetLastError();
}
// The forms that exist (a new one: its struct in mppi_kernels.h and its line here).
#define MPPI_FINISH_FORM(Form) \
  template hipError_t launch_batch_finish<Form>(const FinishArgs&, const BatchArgs&, const Form&, size_t, hipStream_t)
MPPI_FINISH_FORM(BatchPlainRun);
MPPI_FINISH_FORM(BatchIo);
MPPI_FINISH_FORM(BatchTrackedIo);
MPPI_FINISH_FORM(BatchCampaign);
MPPI_FINISH_FORM(BatchScoredCampaign);
MPPI_FINISH_FORM(BatchWheelRun);
MPPI_FINISH_FORM(BatchWheelCampaign);
MPPI_FINISH_FORM(BatchWheelScored);
#undef MPPI_FINISH_FORM
#define MPPI_INGEST_FORM(Form) \
  template hipError_t launch_batch_ingest<Form>(const BatchArgs&, const BatchIo&, const int*, const Form&, hipStream_t)
MPPI_INGEST_FORM(BatchPlainRun);
MPPI_INGEST_FORM(BatchTrack);
MPPI_INGEST_FORM(BatchWheelTrack);
#undef MPPI_INGEST_FORM
template hipError_t launch_batch_claim<BatchCampaign>(const BatchArgs&, const BatchCampaign&, hipStream_t);
template hipError_t launch_batch_claim<BatchScoredCampaign>(const BatchArgs&, const BatchScoredCampaign&, hipStream_t);
