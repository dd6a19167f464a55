// Kernel argument blocks and launchers shared by mppi_kernels.hip and mppi_capi.cpp.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "mppi_cmd.h"

namespace mppi {

constexpr int kTailSlots = 4;  // deferred optimal rollouts in flight (mppi_capi.cpp; 8 / 16 measured
                               // within noise, profiles/r04_notes.md)
constexpr unsigned kDoneFail = 0x80000000u;   // done | kDoneFail: the step's finish gave up
struct FinishArgs {
  int H;
  int mode;  // 0: write root record, 1: finish (u_opt + optimal rollout),
             // 2: finish with the optimal rollout deferred to mppi_tail_kernel (step 0 only here)
  const double* recs;
  int n_recs;
  const float* rec_m;  // [n_recs] the records' m contiguous, or null (read from recs)
  unsigned long long* uopt;  // [2H] colfin: the u_opt handoff words {u bits, seq << 32} (zeroed once)
  double* scratch0;
  double* scratch1;
  double* record_out;  // mode 0
  float T;
  // finish
  float* u_nom_next;  // [2H]
  float* out;         // [16H] u1,u2,v,w,traj,hv,lw,rw
  const float* Z;
  const float4* ntab;  // per-cell normals (see RolloutArgs)
  int rows, grid;
  float x_min, y_min, res;
  float rinv_res;
  int cdiv_res;
  float x0, y0, h0x, h0y, h0z, wl, wr;
  float ok, oa, rwheel, vmin, vmax, wmin, wmax, dt, off;
  // deferred optimal rollout (mode 2 / mppi_tail_kernel)
  float* tail_in;   // [3H] v, sin(w dt), cos(w dt) of the optimal sequence
  float* tail_out;  // [12H] traj, hv, lw, rw (pinned host memory)
  // completion: after every output store, lane 0 stores `seq` to *done (pinned host
  // memory, system scope, release) so the host can spin on it instead of a stream sync
  unsigned* done;
  unsigned seq;
  // resident server: a finish workgroup that gave up stores the step's seq here, and the last finish
  // workgroup's u_opt poll stops on it (null: separate launches)
  unsigned* abort;
  uint64_t* clk;  // optional: the deferred tail's stamps (kClkServer ring)
  // multi-workgroup first tree level (launch_finish with groups > 1)
  double* level1;         // [groups][2H+2]
  unsigned* level1_cnt;   // zero-initialised, re-armed in-kernel
};

struct RolloutArgs {
  // sizes / ids
  int64_t K;         // trajectories in this launch (shard-local)
  int64_t k_offset;  // global index of trajectory 0 (Philox subsequence)
  int H;
  // The critic set (mppi_set_critics) fills the two alignment holes of this block, here and behind
  // `res`, so that no other field's offset moved when it came (the server's argument loads and with
  // them its register allocation stayed what they were).  slope_body: the slope critic on the body
  // path (_avoid_slope, critics_warp.py:131-166: both "wheels" of slope_term on the bilinear body
  // height) instead of the wheel contacts.
  int slope_body;
  // DEM
  const float* Z;
  const float4* ntab;  // per-cell normals [(rows+1) x (grid+1)] (mppi_normal_table_kernel)
  int rows, grid;
  float x_min, y_min, res;
  float w_orient;  // the critic set: weight of _path_orientation_critic (:44-82; 0: the term does not exist)
  // costmap
  const float* cm;
  int cm_size;
  float hw, res_c;
  // verified division-by-constant for grid indices (cdiv_f): reciprocal + enable flag
  float rinv_res, rinv_res_c;
  int cdiv_res, cdiv_res_c;
  // robot / goal state (MPPI_isaac.py:489-497, :611-613)
  float x0, y0, h0x, h0y, h0z, wl, wr, gx, gy, s1, s2;
  // sampling
  uint64_t seed, n_base;  // Philox key, block index of (step, t=0)
  const float* eps;       // pair kernel, MODE 0: this step's normals [blocks][2][H][256] (mppi_noise_kernel)
  const float* u_nom1;
  const float* u_nom2;
  float min_u1, max_u1, min_u2, max_u2;
  // filter (sampling_warp.py:96-138)
  float fk, fa, rwheel, vmin, vmax, wmin, wmax;
  // rollout
  float dt, off;
  // critics (critics_warp.py:85-329); pf_far/igx/igy/pf_scale/speed_on precomputed in f32
  int pf_far, speed_on;
  float igx, igy, pf_scale;
  float w_path, w_slope, w_speed, w_obs, thr, pen, T;
  // outputs
  float* cost_out;   // [K]
  double* nodes;     // [blocks][2H+2]
  float* rec_m;      // [blocks] or null: each record's m again, contiguous (the finish's scale table)
  float* ustore;     // [blocks][2][H][block] sampled controls kept for the weighted sum
  // injected controls (MODE 1), trajectory-major [K*H]
  const float* inj_u1;
  const float* inj_u2;
  // dump (DUMP)
  float *d_traj, *d_hv, *d_lw, *d_rw, *d_v, *d_w, *d_u1, *d_u2;
  int wave_prio;        // pair kernel: raise the waves' issue priority (s_setprio 2)
  int small_angle;      // max(|wmin|, |wmax|) * dt < 0.78: the Rodrigues angle's sin / cos by
                        // dm_sincosf_small (the same bits, no range reduction)
  int ucache_steps;     // pair kernel, MODE 0: steps [0, n) keep their sampled controls in LDS
                        // ([2][n][TB] floats after the scratch) for leaf_records
  // optional [8]: the chain wave of group 0 in workgroup 0 stores s_memtime / s_memrealtime at
  // the start and the end of its H steps ([0..3]: shader clock cycles per step and the clock
  // rate); role-split kernel, workgroup 0: s_memrealtime at its start, when every role is done,
  // and when its leaf record is written ([4..6])
  uint64_t* clk;
};
// clk layout: [0..8) the stamps above, then (role-split kernel) [kClkBase + 2 b], [.. + 1] =
// s_memrealtime when workgroup b (< kClkBlocks) starts and when its record is written
constexpr int kClkBase = 8, kClkBlocks = 4096;
// then (resident server) s_memrealtime per step, ring of 8 steps: [kClkServer + 8 (seq % 8) + k], k =
// 0 the head saw the command, 1 the last rollout ticket, 2 the completion word stored, 3 the
// latest end of a noise share (atomic max), 4 the deferred tail started, 5 the tail ended,
// 6 the head started polling for the command, 7 the latest end of any workgroup's step
// then (resident server, always on) [kClkServer + 64, + 68): the sums of (last ticket - command seen)
// and (completion word - command seen) in 100 MHz ticks, and their step counts
constexpr int kClkServer = kClkBase + 2 * kClkBlocks, kClkSums = kClkServer + 64, kClkWords = kClkSums + 8;
// The finish's phase-2 LDS (finish_phase2): uo[2][PS] v w sin cos[H] chain[12H] out[16H]
// lr[2][PS] floats, PS = the filter rows' stride (a multiple of 4 floats, >= H + 32 for the
// filter's read-ahead).
__host__ __device__ inline int fin_plane_stride(int H) { return ((H + 3) & ~3) + 32; }
__host__ __device__ inline int fin_phase2_floats(int H) { return 4 * fin_plane_stride(H) + 32 * H; }


// The rollout kernel (mppi_rollout_pair_kernel): 256 trajectories per 512-thread workgroup, a
// chain wave and a side wave per 64 trajectories, synchronised through LDS progress counters
// over PAIR_RING-deep rings.
constexpr int PAIR_TRAJ = 256;
// ring depth: round 4, 6 beats 8 at C3 by ~1.4 % (the control cache holds 48 steps instead of 40),
// C4 and the C4 shard unchanged (profiles/r04_notes.md)
constexpr int PAIR_RING = 6;  // = PAIR_D in mppi_kernels.hip
// floats per trajectory and step, side -> chain: (v, sin, cos, 1 - cos) of the Rodrigues angle,
// computed by the side wave at production, off the chain's serial path
constexpr int PAIR_RING_IN = 4;
// the role-split kernel's ring_out depth (x, y, cx, cy of each step, chain -> wheel and cost waves):
// round 6, 8 and 10 (two control-cache steps fewer each) measured within noise of 6 or below it
constexpr int ROLES_RING_OUT = 6;
hipError_t launch_rollout_pair(const RolloutArgs& a, int blocks, size_t lds, hipStream_t st, int proj,
                               int mode, bool dump, bool roles = false);
// The role-split rollout kernel (mppi_rollout_roles_kernel): the same 256 trajectories per
// workgroup over 1024 threads, one wave per role (chain, producer, wheel, cost) and 64
// trajectories; rings [D][4 + 4][TB] + cost[TB] + slope[TB] in LDS.
constexpr int ROLES_WAVES_PER_TRAJ_WAVE = 4;
// The resident step server (mppi_step_server_kernel): one workgroup per 256 trajectories of the
// role-split rollout, resident across steps.  Per step every workgroup waits for a command tagged with
// the next sequence number (or the command's stop slot; the head also leaves after idle_ticks of the 100 MHz
// clock without a command, and the others leave on the stop it relays), runs its rollout and writes its record through, and takes a ticket from rec_cnt;
// the workgroups holding the last fin_groups tickets run the column-split finish (each after rec_cnt
// reaches nroll, or wait_ticks: then the step publishes done | kDoneFail); the other workgroups
// generate the normals of step + 2 meanwhile (ServerCmd::noise_slot, a static share per ticket;
// workgroup 0's first wave keeps out of it).  Only workgroup
// 0 polls the pinned command (256 workgroups polling host memory cost ~30 us per step, one ~4 us:
// profiles/ubench/server.hip); it relays the tagged command slots (mppi_cmd.h) through device memory.
struct ServerArgs {
  FinishArgs f;
  int nroll, fin_P, fin_ncol, fin_groups;
  unsigned* rec_cnt;          // [0] records counted; zeroed, re-armed by the finish
  const ServerCmdWire* cmd;   // pinned host memory (polled by the head only): the tagged command slots
  unsigned long long* relay;  // device [kCmdSlots]: the same slots as relayed by the head, slot kCmdStopSlot
                              // the launch_id of the launch it stopped
  unsigned launch_id;         // unique per launch of the context (never 0): the stop word that ends it
  float* eps[3];              // the normals slots
  float* u_nom[2];            // the nominal double buffer, [2H] each
  float* tail_in[kTailSlots];   // deferred optimal rollout inputs per slot (device)
  float* tail_out[kTailSlots];  // its outputs per slot (pinned)
  unsigned first_seq;
  uint64_t wait_ticks;        // a finish's record wait bound
  uint64_t idle_ticks;        // the head leaves after this long without a command (and relays the stop)
  unsigned exit_after;        // test hook (0: off): the head leaves at its poll after serving this many
                              // commands, whether or not the next one was posted
  unsigned plan;              // the sampling plan's elementwise part for the noise phase: bit 0 antithetic,
                              // bit 1 nominal (in the padding behind exit_after: no other offset moved)
  uint64_t* clk;            // optional: the server stamps [kClkServer, kClkServer + 4) of RolloutArgs::clk
};
hipError_t launch_step_server(const RolloutArgs& a, const ServerArgs& z, size_t lds, hipStream_t st, int proj);
// record tree finish (mppi_finish_kernel): the fallback where the column-split shape does not fit
hipError_t launch_finish(const FinishArgs& f, size_t lds, hipStream_t st, int groups = 1);
// column-split finish: every workgroup builds the pair-scale table and reduces ncol columns
// over all n records; the last to arrive runs phase 2 (f.level1 holds >= 2H floats, f.level1_cnt
// a zeroed counter).  colfin_shape returns 0 when n is outside the kernel's range.
// (at most max_groups workgroups: more columns each).
int colfin_shape(int n, int H, int* P, int* ncol, int* groups, size_t* lds_tree, int max_groups = 1 << 30);
hipError_t launch_colfin(const FinishArgs& f, size_t lds, hipStream_t st, int P, int ncol, int groups);
// optimal rollout of the sequence a mode-2 finish left in f.tail_in (one workgroup)
constexpr int TAIL_THREADS = 256;
hipError_t launch_tail(const FinishArgs& f, hipStream_t st);
// per-cell surface normals of the DEM, [(rows+1) x (grid+1)] float4 (x, y, z, 0)
hipError_t launch_normal_table(const float* Z, int rows, int grid, float res, float4* out, hipStream_t st);
hipError_t launch_selftest(int what, int64_t n, uint64_t seed, unsigned long long* bad, hipStream_t st);
// test hook: `groups` workgroups each holding `lds` bytes of LDS for `ticks` (100 MHz)
hipError_t launch_hold(int groups, size_t lds, uint64_t ticks, hipStream_t st);
// counts the significands a in [1, 2) for which cdiv_f(a, b, y) != a / b (IEEE)
hipError_t launch_cdiv_verify(float b, float y, unsigned* bad, hipStream_t st);
// The sampling normals of one step (Philox block n_base + t/2 of global trajectory k_offset + k),
// laid out [blocks][2][H][256]: eps1 rows then eps2 rows, 256 trajectories per row.
// A sampling plan as the generator takes it: mppi_sampling (include/mppi.h) and g = (float)sqrt(1 -
// beta^2) in float64, formed once on the host (the semantics: mppi_detmath.h).  In the
// batch's table (BatchNoisePlan::rows) antithetic -1 marks a row the caller did not give.
struct SamplePlan {
  int antithetic, nominal;
  float beta, g;
};
// `plan`: the sampling plan; the default plan launches the kernel as it was,
// antithetic / nominal its elementwise form, beta > 0 the serial form (one wave per leaf block and 64
// trajectories, which walks the step's Philox blocks in order).
hipError_t launch_noise(uint64_t seed, uint64_t n_base, int64_t k_offset, int blocks, int H, float* eps,
                        hipStream_t st, int max_groups, const SamplePlan& plan);
// ---- batched closed-loop episodes (mppi_batch_*) ----
// E independent episodes over one context's parameters and (unless an episode holds a scene slot of
// the batch) scene, advanced by three stream-ordered
// launches per step (normals, rollout, finish-and-advance) with the loop's state feedback on the GPU.
// One record per episode in device memory: what a single-context step takes from mppi_state and
// state_fields() (mppi_capi.cpp) as kernel arguments, plus the loop's own counters.
struct BatchEpisode {
  float x0, y0, h0x, h0y, h0z, wl, wr, gx, gy, s1, s2;  // mppi_state
  int pf_far, speed_on;                                 // state_fields(): the critics' scalar parts
  float igx, igy, pf_scale;
  int active;      // runs the next step (runnable and outside the goal tolerance)
  int cur;         // the half of the nominal double buffer the next step reads
  uint64_t seed;   // Philox key
  uint64_t step;   // Philox step index (steps since mppi_batch_set_episode)
  int steps_run;   // steps of the current run = rows in the episode's log
  int reached;     // the goal test passed
};
static_assert(sizeof(BatchEpisode) == 96, "BatchEpisode layout");
// One row of the batch's variant table: mppi_batch_variant (include/mppi.h) field for field.  The
// parameters an episode may override: kernel scalars only, read with wave-uniform loads.
struct BatchVariant {
  float w_path, w_slope, w_speed, w_obs, thr, pen, T, fk, fa, ok, oa, sigma_base, sigma_div;
  int proj;
};
static_assert(sizeof(BatchVariant) == 56, "BatchVariant layout");
constexpr int kBatchMaxVariants = 1024;
// One row of the batch's critic table: mppi_critics (include/mppi.h) field for field.  Row i belongs to
// variant row i; the rows the caller did not give hold slope_mode -1: the context's set, which the
// launch's arguments carry.
struct BatchCriticRow {
  int slope_mode;
  float w_orient;
};
static_assert(sizeof(BatchCriticRow) == 8, "BatchCriticRow layout");
// Per-episode scene and trajectory count (mppi_batch_set_dem / _set_costmap / _set_episode_scene /
// _set_episode_trajectories).  One record per episode, read as one wave-uniform 16-byte load: its
// DEM and costmap slots (-1: the context's) and its K with blocks = ceil(K / 256) (the context's for
// an episode that holds none).  The slots' device pointers are three tables indexed by slot, in
// the same device allocation (BatchSceneTable), so the kernels' arguments carry one pointer.
struct BatchScene {
  int dem, cm, K, blocks;
};
static_assert(sizeof(BatchScene) == 16, "BatchScene layout");
constexpr int kBatchMaxDems = 256;       // DEM slots of a batch (heights + normal table each)
constexpr int kBatchMaxCostmaps = 1024;  // costmap slots of a batch
struct BatchSceneTable {
  const float* dem_z[kBatchMaxDems];      // heights of each DEM slot
  const float4* dem_ntab[kBatchMaxDems];  // its normal table
  const float* cms[kBatchMaxCostmaps];    // each costmap slot
  BatchScene rec[1];                      // [E] the episodes' records
};
struct BatchArgs {
  // null when no set episode holds a variant: the kernels then read no table, and a batch without
  // variants runs as it did before there were any (the index and the row are two dependent loads
  // at the head of the rollout and of the finish: 0.6 us per step measured at K = 1 000, E = 64)
  const BatchVariant* var;  // [kBatchMaxVariants] the variant table
  const int* ep_var;        // [E] each episode's row of the table, -1: none
  // null while no set episode holds a DEM slot, a costmap slot or a K of its own (the variants' rule:
  // such a batch pays one scalar compare per kernel)
  const BatchSceneTable* scene;
  BatchEpisode* ep;  // [E]
  int E, blocks, H;
  int proj;          // the run's projection: that of the episodes without a variant
  int64_t k_pad;     // blocks * 256
  float* eps;        // [E][blocks][2][H][256] this step's normals
  float* unom;       // [E][2][2H] nominal double buffer
  double* nodes;     // [E][blocks][2H + 2] leaf records
  float* cost;       // [E][k_pad]
  float* fin;        // [E][7H + 12]: the mode-2 finish outputs (u1, u2, v, w [H], row 0 [12]), then its
                     // tail inputs [3H] (written by finish_phase2, not read: the loop consumes row 0 only)
  float* log;        // [E][log_cap][8]: x, y, z, heading, v, w per step of the run
  int log_cap;
  float sigma_base, sigma_div, goal_tol;  // mppi_loop_policy (an episode's variant overrides the sigmas)
  float horizon, rwheel;                  // mppi_params horizon, robot_radius
  int* active_count;                      // pinned host memory: episodes still active
  // null while no critic rows are set (mppi_batch_set_variant_critics): [kBatchMaxVariants], read by
  // the rollout only, behind the variant index it has loaded already
  const BatchCriticRow* crit;
};
// (the scene pointer took the place of two paddings: the kernels' argument segment did not grow)
static_assert(sizeof(BatchArgs) == 144, "BatchArgs layout");
constexpr int kBatchMaxRecords = 16;  // leaf records per episode: the finish's tree is one LDS pass
// The noise launch's sampling plans: the context's, and the table of the variant rows' plans
// (mppi_batch_set_variant_sampling; null: none set), [kBatchMaxVariants], read behind the variant index.
struct BatchNoisePlan {
  SamplePlan ctx;
  const SamplePlan* rows;
};
hipError_t launch_batch_noise(const BatchArgs& b, int64_t k_offset, hipStream_t st, const BatchNoisePlan& np);
hipError_t launch_batch_rollout(const RolloutArgs& a, const BatchArgs& b, size_t lds, hipStream_t st, int proj);
// The finish, ingest and claim kernels are templates on a form: a struct that is the kernel's last
// argument, says what it is (kCampaign, kScored, kStep, kTracked, kWheels) and hands out its parts
// (queue(), scored(), io(), track(), wheels(); each exists where its flag is set).  A new form is one
// more struct and one more line of explicit instantiation in mppi_batch_kernels.h; DESIGN.md §3.7 has
// the table.  The static_asserts beside the structs hold the kernel-argument layouts.
struct BatchPlainRun {  // mppi_batch_run, and the ingest of mppi_batch_step_device: no part
  static constexpr bool kCampaign = false, kScored = false, kStep = false, kTracked = false, kWheels = false;
};
// ---- the task queue of a batch (mppi_batch_set_tasks / _run_tasks) ----
// The E episodes become lanes that work through N tasks: the lane whose task ends (goal reached, or
// the task's step cap) writes the task's result and claims the next index of the list with one
// agent-scope atomic add, in the finish kernel's campaign form.  The other kernels do not know:
// they read the lane's BatchEpisode, ep_var[e] and scene->rec[e], which the finish rewrote behind
// a kernel boundary.
struct BatchTask {  // one task as the host resolved it (mppi_batch_task)
  float x0, y0, h0x, h0y, h0z, wl, wr, gx, gy, s1, s2;  // the start, heading as given
  int variant;          // row of the variant table, -1: none
  uint64_t seed;        // Philox key
  BatchScene scene;     // slots (-1: the context's), K and blocks, resolved
  int max_steps;        // >= 1
  int pad;
  int64_t log_base;     // first row of the task in the log arena: the prefix sum of the caps before it
};
static_assert(sizeof(BatchTask) == 88, "BatchTask layout");
struct BatchTaskResult {
  float x0, y0, h0x, h0y, h0z, wl, wr, gx, gy, s1, s2;  // the state after the task's last step
  int steps;    // steps taken = rows of the task in the arena
  int reached;  // the goal test passed
  int flags;    // 1: claimed by a lane, 2: ended
};
static_assert(sizeof(BatchTaskResult) == 56, "BatchTaskResult layout");
struct BatchLane {  // what a lane keeps of its task beside its BatchEpisode: one 16-byte load
  int task;         // index into the list, -1: none
  int max_steps;
  int64_t log_base;
};
static_assert(sizeof(BatchLane) == 16, "BatchLane layout");
struct BatchCampaign {
  const BatchTask* tasks;  // [n]
  BatchTaskResult* res;    // [n]
  BatchLane* lane;         // [E]
  int* next_task;          // the next unclaimed index (may pass n by the number of lanes)
  int* lane_steps;         // [E] the steps each lane has run: lanes run without gaps until the list is
                           // exhausted, so the largest is the campaign's batch steps so far
  float* log;              // [sum of max_steps][8] the arena
  int* ep_var;             // [E] BatchArgs::ep_var, writable
  BatchScene* rec;         // [E] BatchSceneTable::rec, writable
  int n;
  static constexpr bool kCampaign = true, kScored = false, kStep = false, kTracked = false, kWheels = false;
  __host__ __device__ const BatchCampaign& queue() const { return *this; }
};
static_assert(sizeof(BatchCampaign) == 72, "BatchCampaign layout");
// ---- a scored task list (mppi_batch_set_tasks_scored / _get_task_scores) ----
// The advance lane of the finish kernel extends the four critic chains of the log scorer
// (mppi_score_chain.h) by the row it logs, and writes the task's score row with its result: what
// mppi_batch_score_tasks(b, yardstick, NULL, ...) computes from the log, bit for bit, without a log.
// One record per lane: read and written by the advance lane of workgroup e only, reset by the claim,
// which also fills the goal terms of the task's start (the scorer's ScoreGoal).
struct BatchScoreAcc {
  float path, slope, speed, obs;  // the four chains
  float path_pend;                // the near branch's term of the last row: it enters when the next row arrives
  float slope_pend;               // the slope term of the last even row: it enters when the odd row behind it arrives
  int col;                        // collisions
  float pe[3];                    // the previous even waypoint
  float lx, ly;                   // the last row's x, y (the orientation critic reads the last two rows)
  float sx, sy, sz;               // the last sampled waypoint (rows 0, 5, 10, ...) of `length`
  float x0, y0, igx, igy, pf_scale;  // the goal terms of the task's start (state_fields())
  int pf_far, speed_on;
  double length;                  // compute_length of evaluate_trajectory.py:43-53 so far, float64
};
static_assert(sizeof(BatchScoreAcc) == 96, "BatchScoreAcc layout");
struct BatchTaskScore {  // one row per task, zero until the task ends (and for a task that took no step)
  float cost;
  float terms[4];  // path, slope (body form), speed, obstacle
  int collisions;
  int rows;        // = the task's steps
  int pad;
  double length;
};
static_assert(sizeof(BatchTaskScore) == 40, "BatchTaskScore layout");
// What an executed path is scored against: the geometry of the context's costmap as it stands when the run
// or the step is enqueued, and the limits and weights as taken when the list or tracking was set.  (The
// costmap's pointer and size stay beside it in the two forms, where their kernels' arguments have them.)
struct BatchYardstick {
  float hw, res_c;
  float vmax, thr, pen;
  float w_path, w_slope, w_speed, w_obs, w_orient;
};
static_assert(sizeof(BatchYardstick) == 40, "BatchYardstick layout");
// The scored form (BatchArgs does not grow): the queue, the two tables and the yardstick.
struct BatchScoredCampaign {
  BatchCampaign q;          // q.log null: the list keeps no log and no row is written
  BatchScoreAcc* acc;       // [E]
  BatchTaskScore* score;    // [n]
  const float* cm;          // the context's costmap: a task without a costmap slot
  int cm_size;
  BatchYardstick y;
  static constexpr bool kCampaign = true, kScored = true, kStep = false, kTracked = false, kWheels = false;
  __host__ __device__ const BatchCampaign& queue() const { return q; }
  __host__ __device__ const BatchScoredCampaign& scored() const { return *this; }
};
static_assert(sizeof(BatchScoredCampaign) == 144 && offsetof(BatchScoredCampaign, acc) == 72 &&
                  offsetof(BatchScoredCampaign, cm) == 88 && offsetof(BatchScoredCampaign, y.w_orient) == 136,
              "BatchScoredCampaign layout");
// ---- the device-resident step of a batch (mppi_batch_step_device) ----
// One step of every set episode for a plant that is not the controller's own model: the ingest
// kernel writes the caller's states into the episode records, the noise and rollout kernels run as
// in any step, and the finish kernel's step form hands the command and the plan out instead of
// advancing.  mppi_batch_io (include/mppi.h) field for field: device pointers, the step form of the
// finish and the second argument of every ingest (BatchArgs does not grow).
struct BatchIo {
  const float* states;    // [E][11] mppi_state field order
  const int* mask;        // [E] or null
  const int* reset;       // [E] or null
  const uint64_t* seeds;  // [E] or null
  float* cmd;             // [E][2] or null
  float* plan;            // [E][4H + 12] or null
  static constexpr bool kCampaign = false, kScored = false, kStep = true, kTracked = false, kWheels = false;
  __host__ __device__ const BatchIo& io() const { return *this; }
};
static_assert(sizeof(BatchIo) == 48, "BatchIo layout");
// ---- tracked device steps (mppi_batch_set_tracking / _step_tracked) ----
// The device step with the notion of a run: the ingest kernel's tracked form logs the row an ingested
// state makes with the command the previous step wrote, extends the scorer's chains by it as the
// scored campaign's advance lane does, tests the goal and the step cap, and writes the run's result
// and score row when it ends; an ended episode stays inactive until its next reset.
// One record per episode: read and written by lane 0 of workgroup e of the ingest only, but for
// (v, w), which the tracked step finish stores behind a kernel boundary.
struct BatchTrackRec {
  BatchScoreAcc acc;  // the run's chains so far; acc.x0, acc.y0: the run's start
  float gx, gy;       // the run's goal (the start state's)
  float v, w;         // the command the episode's previous step wrote
  float px, py;       // x, y of the row before the last one (acc.lx, acc.ly hold the last row's)
  int rows;           // rows of the run so far
  int ended;          // 0: running, 1: reached, 2: the step cap (what `done` reads)
  int fresh;          // the run's start has not been ingested yet (mppi_batch_set_episode)
  int pad;
};
static_assert(sizeof(BatchTrackRec) == 136, "BatchTrackRec layout");
constexpr int kRunReached = 1, kRunCap = 2, kRunAbandoned = 3;  // BatchRunResult::r.flags, the run's status
struct BatchRunResult {  // one row per (episode, run ordinal), zero until the run ends
  BatchTaskResult r;     // the state at the ending ingest, steps, reached, flags = the status
  BatchTaskScore s;      // zero for a run that took no step
};
static_assert(sizeof(BatchRunResult) == 96, "BatchRunResult layout");
// The tracked form of the ingest: the tables, the step's two optional arrays, the caps and the yardstick
// as taken when tracking was set, and the context's costmap and DEM, which an episode's slots replace.
struct BatchTrack {
  BatchTrackRec* rec;    // [E]
  int* runs;             // [E] runs ended per episode (may pass runs_per_episode: results were dropped)
  BatchRunResult* results;  // [E][runs_per_episode]
  const float* z;        // [E] or null: the plant's pose height; null: the episode's DEM at (x, y)
  int* done;             // [E] or null: BatchTrackRec::ended of every set episode, 0 for one never set
  int max_steps, runs_per_episode, keep_log;
  int cm_size;
  const float* cm;       // the context's costmap: an episode without a costmap slot
  BatchYardstick y;
  const float* Z;        // the context's DEM: an episode without a DEM slot (z null only)
  int rows, grid;
  float x_min, y_min, res;
  static constexpr bool kCampaign = false, kScored = false, kStep = false, kTracked = true, kWheels = false;
  __host__ __device__ const BatchTrack& track() const { return *this; }
};
static_assert(sizeof(BatchTrack) == 136 && offsetof(BatchTrack, cm) == 56 && offsetof(BatchTrack, y.w_orient) == 100 &&
                  offsetof(BatchTrack, Z) == 104,
              "BatchTrack layout");
// The tracked step form of the finish: the io block and the records that take (v, w).
struct BatchTrackedIo {
  BatchIo base;
  BatchTrackRec* rec;  // [E]
  static constexpr bool kCampaign = false, kScored = false, kStep = true, kTracked = true, kWheels = false;
  __host__ __device__ const BatchIo& io() const { return base; }
  __host__ __device__ BatchTrackRec* track() const { return rec; }
};
static_assert(sizeof(BatchTrackedIo) == 56 && offsetof(BatchTrackedIo, rec) == 48, "BatchTrackedIo layout");
// ---- wheel contacts and path metrics of executed paths (mppi_batch_set_wheel_log /
// _set_score_options) ----
// Opt-in: a batch that turns none of them on launches the kernels above with the arguments above.  With
// one on, the host fills the forms below: the form they extend, followed by BatchWheelOpts; every table is
// allocated only while its option is on.
//   wlog     the wheel-contact log, parallel to the log: row n of a path's log has its contacts
//            (lx, ly, lz, rx, ry, rz) in row n of the same index here.  Own model: floats 4H + 6 .. 4H + 11
//            of the step's finish output (row 0 of left_wheel_sim / right_wheel_sim); tracked: formed by
//            the ingest from the ingested pose and the episode's DEM (projection_warp.py:331-347).
//   wacc     the two previous even contacts of each lane: with it the online slope chain is the wheel
//            form (chain::slope_one on both wheels, the larger value), else the body form.
//   macc / metrics  the online state of compute_path_metrics (mppi_path_metrics.h) per lane, and the
//            result rows beside the score rows ([n] tasks, or [E][runs_per_episode]).
struct BatchWheelAcc {
  float pl[3], pr[3];  // the contacts of the last even row
};
static_assert(sizeof(BatchWheelAcc) == 24, "BatchWheelAcc layout");
struct PathMetricsAcc;
struct PathMetrics;
struct BatchWheelOpts {
  float* wlog;           // null: no wheel log (a list or tracking that keeps no log has none either)
  BatchWheelAcc* wacc;   // [E] or null
  PathMetricsAcc* macc;  // [E] or null
  PathMetrics* metrics;  // with macc
  float off;             // mppi_params wheel_offset (the tracked ingest forms the contacts)
  int pad;
};
static_assert(sizeof(BatchWheelOpts) == 40, "BatchWheelOpts layout");
struct BatchWheelRun {  // the plain finish form's (mppi_batch_run with the wheel log on)
  BatchWheelOpts x;
  static constexpr bool kCampaign = false, kScored = false, kStep = false, kTracked = false, kWheels = true;
  __host__ __device__ const BatchWheelOpts& wheels() const { return x; }
};
static_assert(sizeof(BatchWheelRun) == 40, "BatchWheelRun layout");
struct BatchWheelCampaign {
  BatchCampaign q;
  BatchWheelOpts x;
  static constexpr bool kCampaign = true, kScored = false, kStep = false, kTracked = false, kWheels = true;
  __host__ __device__ const BatchCampaign& queue() const { return q; }
  __host__ __device__ const BatchWheelOpts& wheels() const { return x; }
};
static_assert(sizeof(BatchWheelCampaign) == 112 && offsetof(BatchWheelCampaign, x) == 72, "BatchWheelCampaign layout");
struct BatchWheelScored {
  BatchScoredCampaign s;
  BatchWheelOpts x;
  static constexpr bool kCampaign = true, kScored = true, kStep = false, kTracked = false, kWheels = true;
  __host__ __device__ const BatchCampaign& queue() const { return s.q; }
  __host__ __device__ const BatchScoredCampaign& scored() const { return s; }
  __host__ __device__ const BatchWheelOpts& wheels() const { return x; }
};
static_assert(sizeof(BatchWheelScored) == 184 && offsetof(BatchWheelScored, x) == 144, "BatchWheelScored layout");
struct BatchWheelTrack {
  BatchTrack t;
  BatchWheelOpts x;
  static constexpr bool kCampaign = false, kScored = false, kStep = false, kTracked = true, kWheels = true;
  __host__ __device__ const BatchTrack& track() const { return t; }
  __host__ __device__ const BatchWheelOpts& wheels() const { return x; }
};
static_assert(sizeof(BatchWheelTrack) == 176 && offsetof(BatchWheelTrack, x) == 136, "BatchWheelTrack layout");
// One launcher per kernel, defined and explicitly instantiated for the forms above in mppi_batch_kernels.h.
template <class Form>
hipError_t launch_batch_finish(const FinishArgs& f, const BatchArgs& b, const Form& form, size_t lds, hipStream_t st);
// is_set: [E] the host's "mppi_batch_set_episode was called" flags in device memory
template <class Form>
hipError_t launch_batch_ingest(const BatchArgs& b, const BatchIo& io, const int* is_set, const Form& form,
                               hipStream_t st);
// The first fill of a task list: E workgroups claim as a finishing lane does (one statement of the rule).
template <class Form>
hipError_t launch_batch_claim(const BatchArgs& b, const Form& form, hipStream_t st);

hipError_t launch_bilinear(const float* Z, int rows, int grid, float x_min, float y_min, float res,
                           const float* xs, const float* ys, float* hs, int64_t n, hipStream_t st);
// LDS-tiled lookup over queries binned by BIL_TILE x BIL_TILE-cell DEM tile (tile count =
// ceil(rows/BIL_TILE) * ceil(cols/BIL_TILE); the binning keeps one LDS counter per tile, so
// mppi_bin_queries refuses DEMs with more than ~40 000 tiles, e.g. a skinny 2 x 2^24 grid).  Binning: G chunks of
// the queries, each one workgroup with an LDS histogram (hist[G][ntiles] scratch), the tile
// counts' exclusive scan, then the scatter: with <= 4096 tiles and the level-1 scratch (cx, cy, ci
// [n], bcur [tile rows]) two levels of LDS-sorted runs (by tile row into cx/cy/ci, then by tile),
// else each chunk straight from the tile cursors; perm int32 (n < 2^31).
constexpr int BIL_TILE = 128;
int bin_chunks(int64_t n, int ntiles);  // G for n queries
hipError_t launch_bin_queries(const float* xs, const float* ys, int64_t n, float x_min, float y_min, float res,
                              float rinv, int cdiv, int rows, int grid, int* hist, int* counts, int* cursor,
                              int* off, float* xs_out, float* ys_out, int32_t* perm, hipStream_t st,
                              float* cx, float* cy, int32_t* ci, int* bcur);
hipError_t launch_bilinear_tiled(const float* Z, int rows, int grid, float x_min, float y_min, float res,
                                 float rinv, int cdiv, const float* xs, const float* ys, float* hs,
                                 const int* tile_off, hipStream_t st);

}  // namespace mppi
