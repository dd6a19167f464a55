/*
 * mppi.h — C-ABI of the MI355X MPPI rollout-and-cost engine (libmppi_hip.so).
 *
 * Drop-in boundary for the Warp MPPI step of
 * thesis_master/warp_implementation/MPPI_isaac.py (reference, read-only).
 * Plain C types only: host pointers + sizes, device pointers only where the
 * caller already owns device memory (zero-copy DEM binding, rank records).
 *
 * Conventions
 *   status:   every int-returning call returns MPPI_OK (0) or a negative
 *             code; mppi_last_error() (thread-local) holds the message.
 *   memory:   the caller owns host buffers (copied in/out); the library owns
 *             its device buffers and pinned staging.
 *   threads:  one context per device; calls on one context are serialised
 *             by the caller (the reference is single-threaded, driven from
 *             the Isaac main loop, visual_terrain_stack_full_terrain.py:466).
 *   sync:     mppi_step / mppi_step_finish / mppi_step_injected return with
 *             the outputs in host memory (the reference's .numpy() reads,
 *             MPPI_isaac.py:769-775 / visual_terrain_stack_full_terrain.py:471-472).
 */
#ifndef HUSKY_MPPI_H
#define HUSKY_MPPI_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MPPI_ABI_VERSION 1

enum mppi_status {
  MPPI_OK = 0,
  MPPI_EINVAL = -1, /* bad argument (reference: Warp raises on bad launch inputs) */
  MPPI_EHIP = -2,   /* HIP runtime error (device fault, OOM, no device) */
  MPPI_ESTATE = -3, /* call out of order (e.g. step before set_dem) */
};

enum mppi_proj {
  MPPI_PROJ_2D = 2, /* projection_warp.py:353-382 (_generate_trajectories_2D_kernel) */
  MPPI_PROJ_3D = 3, /* projection_warp.py:284-350 (_generate_trajectories_kernel)    */
};

typedef struct mppi_ctx mppi_ctx;

/* Controller parameters.  Replaces MPPI_Controller.__init__ config parsing
 * (MPPI_isaac.py:404-440, config.yaml) and the constants hard-coded at
 * MPPI_isaac.py:548-549,688-689, projection_warp.py:333,
 * critics_warp.py:251-253,325-329.  Float fields are used as float32, the
 * precision the Warp kernels receive them in. */
typedef struct mppi_params {
  int64_t num_trajectories; /* trajectories of THIS context (its shard of K)         */
  int64_t k_offset;         /* global index of this shard's first trajectory          */
  int32_t num_iterations;   /* H (config.yaml controller.number_of_iterations)        */
  int32_t reserved0;
  float dt;                 /* config.yaml controller.dt                              */
  float robot_radius;       /* r_wheels of _convert_inputs_to_velocities (frame_work.robot_radius) */
  float min_u1, max_u1, min_u2, max_u2;                    /* config.yaml inputs.*       */
  float v_min_linear, v_max_linear, v_min_angular, v_max_angular; /* velocities.*        */
  float temperature;        /* cost_evaluation.temperature                            */
  float filter_k, filter_a;         /* rollout wheel filter, MPPI_isaac.py:548-549 (3.5, 0.96) */
  float opt_filter_k, opt_filter_a; /* optimal-sequence filter, MPPI_isaac.py:688-689 (3.0, 0.92) */
  float wheel_offset;       /* projection_warp.py:333 (0.2)                           */
  float w_path, w_slope, w_speed, w_obstacle; /* critics_warp.py:325-329               */
  float collision_threshold, collision_penalty; /* critics_warp.py:251-253 (0.99, 1e5) */
  float horizon;            /* MPPI_isaac.py:440 dt*v_max*H (computed by the caller in float64) */
  uint64_t seed;            /* Philox key (replaces default_rng(42).integers, MPPI_isaac.py:409,517); all 64
                               bits are key bits, as all 64 of k_offset + trajectory are counter bits (D14) */
} mppi_params;

/* Per-step robot / goal state: the values MPPI_step reads from the controller
 * (MPPI_isaac.py:489-503 reset("controller"), :538-539, :611-613, :510-511 of
 * the Isaac loop).  heading is normalised by the caller (MPPI_isaac.py:493). */
typedef struct mppi_state {
  float x, y;
  float heading[3];
  float left_wheel_speed, right_wheel_speed;
  float goal_x, goal_y;
  float std_dev_u1, std_dev_u2;
} mppi_state;

/* Host output pointers (any may be NULL).  Each replaces one Warp array the
 * caller reads with .numpy() after MPPI_step (MPPI_isaac.py:446-487). */
typedef struct mppi_outputs {
  float* u1_opt;          /* [H]   optimal_u1_wp                         */
  float* u2_opt;          /* [H]   optimal_u2_wp                         */
  float* lin_vel;         /* [H]   optimal_lin_vel_wp                    */
  float* ang_vel;         /* [H]   optimal_ang_vel_wp                    */
  float* traj_sim;        /* [H*3] trajectories_sim                      */
  float* heading_sim;     /* [H*3] heading_vectors_sim                   */
  float* left_wheel_sim;  /* [H*3] left_wheel_pos_sim                    */
  float* right_wheel_sim; /* [H*3] right_wheel_pos_sim                   */
} mppi_outputs;

int mppi_abi_version(void);
const char* mppi_last_error(void);

/* MPPI_Controller.__init__ + warp_setup (MPPI_isaac.py:404-487): allocate
 * device buffers on `device`; nominal controls start at zero (:446-447). */
int mppi_create(const mppi_params* params, int32_t device, mppi_ctx** out);
void mppi_destroy(mppi_ctx* ctx);

/* Run on the caller's HIP stream (e.g. torch.cuda.current_stream()); NULL = own stream. */
int mppi_set_stream(mppi_ctx* ctx, void* hip_stream);

/* self.Z_wp = wp.array(surface.Z.flatten()) (MPPI_isaac.py:460): copies the
 * row-major rows x cols DEM to the device.  x_min = y_min = -half_width and
 * resolution = 2*half_width/grid_size as in the launch args (:560-564).
 * Any other placement is allowed, rows and cols need not be equal: the cell of
 * (x, y) is column trunc((x - x_min) / resolution) and row
 * -trunc((y + y_min) / resolution), both clamped into the map, so column 0
 * starts at x = x_min and row 0 lies at y = -y_min with y falling as rows grow.
 * rows * cols < 2^29 (MPPI_EINVAL otherwise). */
int mppi_set_dem(mppi_ctx* ctx, const float* z_host, int32_t rows, int32_t cols, float x_min,
                 float y_min, float resolution);

/* controller.Z_wp = DEM_warp rebinding (visual_terrain_stack_full_terrain.py:567):
 * binds a DEM already resident in device memory (zero copy; the caller keeps
 * it alive while steps run).  Waits for every stream of the device (the DEM may
 * have been written on any of them), then derives the per-cell normal table the
 * rollout reads from it. */
int mppi_set_dem_device(mppi_ctx* ctx, const float* z_device, int32_t rows, int32_t cols,
                        float x_min, float y_min, float resolution);

/* The bound DEM was written in place (the terrain manager's dem_wp.assign(...),
 * geometry_clipmaps.py:293): waits for every stream of the device and rebuilds
 * the per-cell normal table from the current heights.  The reference's kernels
 * read the live DEM at every step; here the table is derived, so an in-place
 * write without this call (or a rebinding) leaves the normals of the old
 * heights.  MPPI_EINVAL when no DEM is bound. */
int mppi_dem_updated(mppi_ctx* ctx);

/* self.costmap_wp (MPPI_isaac.py:461) / costmap_wp.assign(...)
 * (visual_terrain_stack_full_terrain.py:563): size x size row-major costmap;
 * half_width and costmap resolution as passed at MPPI_isaac.py:622-624. */
int mppi_set_costmap(mppi_ctx* ctx, const float* costmap_host, int32_t size, float half_width,
                     float resolution);

/* ---- on-device obstacle costmap ----
 * Surface.create_obstacles_costmap(obstacles, origin) (MPPI_isaac.py:361-378),
 * re-run by the Isaac loop on every high-resolution block change and then
 * uploaded with costmap_wp.assign (visual_terrain_stack_full_terrain.py:561-563).
 * obstacles: n rows of (x_global, y_global, r_obs) float64, host memory.  Per
 * obstacle the disc x_local = y_global - y0, y_local = x_global - x0, radius
 * r_obs/2 + r_robot + 0.1 is marked on the size x size grid
 * X, Y = meshgrid(linspace(-half_width, half_width, size)) (float64, as the
 * reference); then the distance to the nearest marked cell, min-max normalised,
 * (1 - d)^power (the reference: 20), float32.  metric MPPI_COSTMAP_CHAMFER5 (the
 * reference's cv2.distanceTransform(DIST_L2, 5), :374): OpenCV's published
 * 5x5 chamfer (distanceTransform_5x5, 16.16 fixed point; computed as 16
 * independent line scans), cv2.normalize NORM_MINMAX as
 * OpenCV 4.x's float32 path (float scale / shift, one fma), (1 - d) in
 * float32, the power correctly rounded (oracle/costmap_ref.py; parity
 * unpinned: cv2 is unavailable).  MPPI_COSTMAP_CHAMFER5_RASTER: the same map
 * by the two row-serial raster passes on one workgroup (diagnostic / A-B).
 * MPPI_COSTMAP_EXACT: exact Euclidean distance, float64 normalise + power, one
 * rounding; no obstacle at all gives an all-1 map.
 * 2 <= size <= 8192.
 *
 * mppi_build_costmap builds straight into the context's costmap (what the
 * reference's create + assign pair leaves in costmap_wp; resolution becomes
 * 2*half_width/size, MPPI_isaac.py:272) and, if out_host != NULL, also copies
 * it to out_host [size*size] (the ndarray the reference returns).  Synchronous.
 * The builder object does the same without a controller context. */
enum mppi_costmap_metric {
  MPPI_COSTMAP_CHAMFER5 = 0, /* cv2.distanceTransform(DIST_L2, 5), MPPI_isaac.py:374 (default) */
  MPPI_COSTMAP_EXACT = 1,    /* exact Euclidean distance transform */
  MPPI_COSTMAP_CHAMFER5_RASTER = 2, /* CHAMFER5 by the raster passes (same result, slower) */
};
typedef struct mppi_costmap_builder mppi_costmap_builder;
int mppi_build_costmap(mppi_ctx* ctx, const double* obstacles, int32_t n, int32_t size,
                       double half_width, double origin_x, double origin_y, double r_robot,
                       int32_t power, float* out_host, int32_t metric);
int mppi_costmap_builder_create(int32_t device, mppi_costmap_builder** out);
void mppi_costmap_builder_destroy(mppi_costmap_builder* b);
/* out_host [size*size] (host) or out_device [size*size] (device memory); either may be NULL. */
int mppi_costmap_builder_build(mppi_costmap_builder* b, const double* obstacles, int32_t n,
                               int32_t size, double half_width, double origin_x, double origin_y,
                               double r_robot, int32_t power, float* out_host, float* out_device,
                               int32_t metric);
/* Device time (HIP events) of the builder's last build, in milliseconds. */
int mppi_costmap_builder_last_ms(mppi_costmap_builder* b, double* ms);

/* ---- hazard costmap: steep terrain joins the rocks ----
 * The thesis's terrain scenarios ("keep avoiding steep craters, but tolerate small ones and gentle
 * inclines") as the controller's hard constraint: the steep cells of a DEM that is already on the
 * device become occupied cells of the obstacle costmap, in the same pass that rasters the rocks.
 *
 * Steep: DEM cell (j, i) is steep iff !(nz >= c), nz the z component of the normal the rollout reads
 * when it stands in that cell (entry (j + 1, i + 1) of the normal table, the same float32 operations)
 * and c = (float)cos(max_slope_deg pi / 180); a NaN nz (non-finite heights) is steep.
 * Which costmap cell: the frame of the rollout's own costmap lookup (column from x + half_width,
 * row from -y + half_width; NOT the axis-swapped origin frame of the rock list), at the cell's
 * centre: with rc = 2 half_width / size, in float64,
 *   column floor((x_min + (i + 0.5) res + half_width) / rc),
 *   row    floor((half_width - (-y_min - (j + 0.5) res)) / rc);
 * a DEM cell whose index falls outside [0, size) is dropped.
 * H0: costmap cells that collected >= min_cells steep cells.  H1: cells whose exact squared cell
 * distance to the nearest H0 cell is <= T = floor((inflate / rc)^2) (H0 empty: H1 empty; inflate
 * = 0: H1 = H0).  Occupancy = H1 | rock discs; distance, normalisation and power as before, for
 * every metric.  No occupied cell at all gives what the rock-only build gives.
 *
 * hz == NULL makes each function exactly its counterpart above.  MPPI_EINVAL, naming the field:
 * max_slope_deg not finite or outside (0, 90), inflate not finite or negative, T beyond int32,
 * min_cells < 1, reserved != 0.  MPPI_ESTATE: no DEM bound / the named DEM slot is empty.
 * mask_host [size*size] (may be NULL): bit 0 H0, bit 1 H1, bit 2 inside a rock disc.
 * mppi_build_costmap_hazard reads the context's bound DEM in place, owned or borrowed
 * (mppi_set_dem_device).  The builder object takes the heights as a device pointer with their
 * geometry (rows x cols float32, row-major); mppi_costmap_builder_last_ms covers the hazard passes.
 * A costmap is a snapshot: mppi_dem_updated and a DEM rebinding do not rebuild it.  The caller
 * rebuilds after the terrain changed. */
typedef struct mppi_hazard {
  float   max_slope_deg; /* cells steeper than this are no-go; in (0, 90) */
  float   inflate;       /* metres the steep region is grown by (the reference's rock margin: r_robot + 0.1) */
  int32_t min_cells;     /* steep DEM cells a costmap cell must collect; >= 1 */
  int32_t reserved;      /* 0 */
} mppi_hazard;
int mppi_build_costmap_hazard(mppi_ctx* ctx, const double* obstacles, int32_t n, int32_t size,
                              double half_width, double origin_x, double origin_y, double r_robot,
                              int32_t power, const mppi_hazard* hz, float* out_host, uint8_t* mask_host,
                              int32_t metric);
int mppi_costmap_builder_build_hazard(mppi_costmap_builder* b, const double* obstacles, int32_t n,
                                      int32_t size, double half_width, double origin_x, double origin_y,
                                      double r_robot, int32_t power, const float* z_device, int32_t rows,
                                      int32_t cols, float x_min, float y_min, float resolution,
                                      const mppi_hazard* hz, float* out_host, float* out_device,
                                      uint8_t* mask_host, int32_t metric);
/* Device time (HIP events) of the steep-cell count kernel alone in the builder's last build, in
 * milliseconds: the one pass over the heights (0 after a build without hz). */
int mppi_costmap_builder_hazard_count_ms(mppi_costmap_builder* b, double* ms);

/* ---- on-device crater-field DEM ----
 * Surface.create_surface(bumps) (MPPI_isaac.py:307-356) on the GPU.  craters: n rows of
 * (cx, cy, height, width) float64, host memory: bump_center, bump_height, bump_width of the
 * reference's list.  The grid is X, Y = meshgrid(linspace(-half_width, half_width, grid_size))
 * (float64: x_j = j * step + (-half_width), step = 2 half_width / (grid_size - 1), the last point
 * half_width itself; row i of the array lies at y_i = x_i).  Each crater is the two gaussians of
 * :319-320, (height - 0.5) exp(-r2 / (2 width^2)) - (height + 0.5) exp(-r2 / (2 (width/2)^2)),
 * each evaluated as the product exp(-(y_i - cy)^2 / s) exp(-(x_j - cx)^2 / s) of a row and a column
 * factor, so the field is one [grid x 2n] . [2n x grid] float64 product (no crater is culled; the
 * order of the sum is the kernel's).  base_host, if given, is added in float64; the sum is rounded
 * once to float32.  n = 0 gives the base, or zeros.  Not bitwise the reference (its exp of the sum,
 * its crater order): at most one float32 ulp apart, on about one cell in 10^5.
 * MPPI_EINVAL, naming the crater and the field, for a non-finite cx, cy, height or width, a zero
 * width (or one whose square under- or overflows), grid_size < 2 (or above 32768), and a half_width
 * that is not finite and > 0.  All calls are synchronous. */
enum mppi_dem_variant { MPPI_DEM_MFMA = 0, MPPI_DEM_VALU = 1 };  /* same result up to the summation order */
typedef struct mppi_dem_builder mppi_dem_builder;
int  mppi_dem_builder_create(int32_t device, mppi_dem_builder** out);
void mppi_dem_builder_destroy(mppi_dem_builder* b);
/* craters: n rows of (cx, cy, height, width) float64, host.  base_host: NULL or [grid*grid] float32.
 * out_host / out_device [grid*grid] float32, either may be NULL. */
int  mppi_dem_builder_build(mppi_dem_builder* b, const double* craters, int32_t n, int32_t grid_size,
                            double half_width, const float* base_host, float* out_host, float* out_device,
                            int32_t variant);
int  mppi_dem_builder_last_ms(mppi_dem_builder* b, double* ms);   /* HIP events, factor + product */
/* Test hook: the product kernel alone on factor tables the caller supplies in device memory, both
 * term-major [terms][grid_size] float64 (r_dev[t][i] the row factors, c_dev[t][j] the column
 * factors), terms a multiple of 4: out[i][j] = float32(sum_t r_dev[t][i] c_dev[t][j]).  With
 * integer-valued factors every entry is exact, which pins the MFMA lane maps. */
int  mppi_dem_builder_product(mppi_dem_builder* b, const double* r_dev, const double* c_dev, int32_t terms,
                              int32_t grid_size, float* out_host, float* out_device, int32_t variant);
/* create_surface + mppi_set_dem without the host round trip: builds into the context's own DEM buffer with
 * rows = cols = grid_size, x_min = y_min = -(float)half_width, resolution = (float)(2*half_width/grid_size)
 * (MPPI_isaac.py:265, :560-564), then the normal table and the verified reciprocal, as mppi_set_dem.
 * A DEM borrowed by mppi_set_dem_device is let go of, not written into. */
int  mppi_build_dem(mppi_ctx* ctx, const double* craters, int32_t n, int32_t grid_size, double half_width,
                    const float* base_host, float* out_host, int32_t variant);

/* reset("controller") (MPPI_isaac.py:489-497) + the robot/goal/sigma fields MPPI_step reads. */
int mppi_set_state(mppi_ctx* ctx, const mppi_state* state);

/* optimal_u1_wp / optimal_u2_wp as the next step's nominal sequence (MPPI_isaac.py:518-519). */
int mppi_set_nominal(mppi_ctx* ctx, const float* u1, const float* u2);
int mppi_get_nominal(mppi_ctx* ctx, float* u1, float* u2);

/* MPPI_step(proj) (MPPI_isaac.py:505-720) for a single-rank controller:
 * sample -> filter -> rollout -> critics -> softmax-weighted update -> optimal
 * filter -> optimal (3D) rollout; outputs copied to host.  `step` is the
 * Philox step counter (noise offset); the new nominal sequence replaces the
 * old one, as reset("sim") + _compute_weighted_sum do (:655-670).  Any uint64_t
 * is a step: the counter word step * ceil(H/2) + t/2 is taken modulo 2^64 and
 * the step after 2^64 - 1 is step 0. */
int mppi_step(mppi_ctx* ctx, int32_t proj, uint64_t step, mppi_outputs* out);

/* Same with caller-supplied sampled controls u1,u2 [K*H] trajectory-major
 * (the injected-input experiment of compare_3d_2d.py:324-533,668-688). */
int mppi_step_injected(mppi_ctx* ctx, int32_t proj, const float* u1_host, const float* u2_host,
                       mppi_outputs* out);

/* Deferred optimal rollout.  With enable != 0, mppi_step / mppi_step_finish /
 * mppi_step_injected return as soon as the control outputs are in host memory:
 * u1_opt, u2_opt, lin_vel, ang_vel in full and ROW 0 of traj_sim, heading_sim,
 * left_wheel_sim, right_wheel_sim (the pose MPPI_Controller.run consumes,
 * MPPI_isaac.py:769-773).  The rest of the optimal rollout
 * (MPPI_isaac.py:696-720) runs on a side stream, overlapping whatever the
 * caller enqueues next (typically the next step's rollout), and its rows are
 * copied to pinned host memory; mppi_get_outputs waits for it.  Values are
 * bitwise identical to the synchronous mode (enable = 0, the default). */
int mppi_set_async_tail(mppi_ctx* ctx, int32_t enable);
/* All outputs of the last step (waits for a deferred optimal rollout). */
int mppi_get_outputs(mppi_ctx* ctx, mppi_outputs* out);

/* ---- K-sharded multi-GPU step (no reference equivalent) ----
 * Record = [m, S, V1[H], V2[H]] float64 (mppi_record_len() doubles).
 * mppi_step_partial enqueues this rank's rollout and writes its record to
 * record_dev (device memory, async on the context stream); the caller
 * all-gathers the G records (RCCL) and mppi_step_finish combines them in rank
 * order and runs the optimal rollout, returning outputs in host memory. */
int64_t mppi_record_len(mppi_ctx* ctx);
int mppi_step_partial(mppi_ctx* ctx, int32_t proj, uint64_t step, double* record_dev);
int mppi_step_finish(mppi_ctx* ctx, const double* records_dev, int32_t n_records,
                     mppi_outputs* out);

/* ---- the same sharded step driven from ONE process ----
 * For a host that owns several GPUs in one process (the reference's
 * controller object, MPPI_isaac.py:397-470, is single-process; a caller that
 * wants one controller over n GPUs without torch.distributed).  The group
 * holds one context per member device, member i over trajectories
 * [begin_i, begin_i + count_i) of params->num_trajectories (256-trajectory
 * leaves split contiguously, as mppi_amd/distributed.shard_bounds), noise
 * keyed by the global trajectory index.  When every member's shard is a
 * power-of-two number of leaves (e.g. C4's 8 x 512) the member roots are
 * subtrees of the one-context record tree and a group step is bitwise equal
 * to one context over all K; other splits (3 members, ragged K) run the same
 * float64 combine with a different pairing (D2 in DESIGN.md).
 * mppi_group_step runs every member's rollout and record (members 1..n-1 on
 * threads of the group, member 0 on the caller's), all-gathers the records
 * (RCCL ncclAllGather, one communicator per member from ncclCommInitAll,
 * RCCL opened with dlopen, when the devices are distinct; device-to-device
 * copies when members share a device), runs every member's finish and
 * returns member 0's outputs; every member keeps the same nominal controls.
 * Scene, state, weights and warm starts are set on each member through
 * mppi_group_context with the single-context calls above (not while a
 * group step runs). */
typedef struct mppi_group mppi_group;
int mppi_group_create(const mppi_params* params, int32_t n, const int32_t* devices,
                      mppi_group** out);
void mppi_group_destroy(mppi_group* group);
int mppi_group_size(mppi_group* group);
int mppi_group_context(mppi_group* group, int32_t member, mppi_ctx** out);
int mppi_group_shard(mppi_group* group, int32_t member, int64_t* begin, int64_t* count);
int mppi_group_step(mppi_group* group, int32_t proj, uint64_t step, mppi_outputs* out);
/* Group facts, up to 7 values: info[0] = members, [1] = distinct devices, [2] = 1 if the records
 * travel by RCCL (else device copies), [3] = ranks of the RCCL communicator (ncclCommCount; 0
 * without RCCL), [4] = 1 if members 1..n-1 run on group threads, [5] = microseconds a member
 * thread spins for the next step before it sleeps (0 when the members outnumber the granted
 * CPUs), [6] = CPUs this process is granted (affinity, bounded by the cgroup quota). */
int mppi_group_info(mppi_group* group, int64_t* info, int32_t n);
/* Host-only test of the group's member threads (no device work, no GPU needed): n members whose
 * steps take ~20 us of host time, member fail_member's fail (fail_member >= n: none), `steps` group
 * steps.  Every step must return (no member thread left waiting), with the failing member named in
 * mppi_last_error.  info[5]: steps returned, steps failed, failures naming the member, worker
 * threads, spin microseconds. */
int mppi_group_selftest(int32_t n, int32_t fail_member, int32_t steps, int64_t* info);

/* ---- introspection (self.costs_wp / self.trajectories .numpy(), MPPI_isaac.py:466-470) ---- */
/* costs of the last step's trajectories of this context [n <= K] */
int mppi_get_costs(mppi_ctx* ctx, float* costs_host, int64_t n);
/* re-run the last step with per-rollout-step outputs (bitwise identical; [K*H] / [K*H*3]
 * trajectory-major like the reference arrays); any pointer may be NULL. */
int mppi_dump_rollouts(mppi_ctx* ctx, float* traj, float* heading, float* left_wheel,
                       float* right_wheel, float* lin_vel, float* ang_vel, float* u1, float* u2);

/* ---- the critic set ----
 * The evaluation kernel (critics_warp.py:322-329) is a menu of critic lines that the thesis switched
 * in and out.  Beside the four of mppi_params' weights two more can be chosen per context:
 *   slope_mode     MPPI_SLOPE_WHEELS: _avoid_slope_wheels over the wheel contacts (:327, the default);
 *                  MPPI_SLOPE_BODY: _avoid_slope over the body path (:326, :131-166): for t = 0, 2, ..
 *                  < H - 3, (1 + 5 |dz / (sqrt(dx dx + dy dy) + 1e-6)|)^2 between waypoints t and t + 2
 *                  of the rollout, z the bilinear height at the body position.  The 2D projection has no
 *                  wheel contacts (they are DEFINED zero), so this is its only slope information.  The
 *                  dumped wheel arrays of a 3D step stay the contacts in either mode.
 *   w_orientation  weight of _path_orientation_critic (:324, :44-82); 0 (the default): no such term.
 *                  xd = goal_x - x, yd = goal_y - y (the robot), (x2, y2) = X[H-1] - X[H-2] of the
 *                  rollout, s = xd x2 + yd y2, po = s <= 0 ? -s / (|xd| + |yd|) : 0, DEFINED 0 where
 *                  |xd| + |yd| == 0 (and for a scored path of one waypoint).
 * The cost is, in float32 and this order, c = w_orientation po (only when the weight is not 0),
 * c += w_path path, c += w_slope slope, c += w_speed speed, c += w_obstacle obstacle.  With the
 * default set every result keeps its bits.
 * mppi_set_critics stops the resident server like every call outside the step set; the set then
 * applies to mppi_step, _step_injected, _step_partial (each group member is set through
 * mppi_group_context), mppi_get_costs, mppi_get_cost_terms and the scoring calls.  MPPI_EINVAL,
 * naming the field, for an unknown mode, a non-finite weight, or w_orientation != 0 with
 * num_iterations < 2. */
enum mppi_slope_mode { MPPI_SLOPE_WHEELS = 0, MPPI_SLOPE_BODY = 1 };
typedef struct mppi_critics { int32_t slope_mode; float w_orientation; } mppi_critics;  /* 8 bytes */
int mppi_set_critics(mppi_ctx* ctx, const mppi_critics* critics);   /* default {WHEELS, 0} */
int mppi_get_critics(mppi_ctx* ctx, mppi_critics* out);

/* ---- the sampling plan ----
 * How the K control sequences of a step are drawn: u = clamp(u_nom[min(t+1, H-1)] + sigma e[k, t, c])
 * with e made of the base normals z[k, t, c] (Philox key = seed, block step * ceil(H/2) + t/2,
 * global trajectory k: unchanged).  src(k) = k & ~1 if `antithetic`, else k.  All float32, no
 * contraction, in this order:
 *   beta        in [0, 1): time-correlated (AR(1)) noise.  e[0] = z[src(k), 0, c], e[t] = (beta e[t-1])
 *               + (g z[src(k), t, c]), three roundings, g = (float)sqrt(1.0 - (double)beta (double)beta).
 *               0: e = z.
 *   antithetic  an odd global k takes -e of k - 1 (an exact sign flip, both channels; its own Philox
 *               stream is unused).  An even k keeps its own draw, with or without a partner.  Needs an
 *               even k_offset.
 *   nominal     global k == 0 gets +0.0f for every t and c: it rolls out the clamped shifted nominal
 *               sequence.  With `antithetic`, k == 1 is the negation of k = 0's un-zeroed sequence.
 * With the default plan {0, 0, 0} every result keeps its bits.  mppi_set_sampling stops the resident
 * server like every call outside the step set and drops the normals generated ahead; the plan applies
 * from the next mppi_step / _step_partial and to mppi_dump_rollouts' re-run of a step taken under it.
 * mppi_step_injected ignores it.  `antithetic` and `nominal` run on the resident server; with beta > 0
 * the steps are separate launches (the generator's serial form does not fit the server's static
 * shares).  Each group member is set through mppi_group_context.  MPPI_EINVAL, naming the field, for a
 * flag outside {0, 1}, a beta that is not finite or outside [0, 1), or antithetic with an odd k_offset. */
typedef struct mppi_sampling { int32_t antithetic; int32_t nominal; float beta; } mppi_sampling;  /* 12 bytes */
int mppi_set_sampling(mppi_ctx* ctx, const mppi_sampling* plan);   /* default {0, 0, 0.0f} */
int mppi_get_sampling(mppi_ctx* ctx, mppi_sampling* out);

/* ---- path scoring and per-critic terms ----
 * _evaluate_trajectories_kernel (critics_warp.py:302-329) on paths the caller supplies: the
 * offline re-scoring of logged runs (evaluate_trajectory.py, dim = 1, paths of up to 3500
 * waypoints) and the cost of the chosen plan (MPPI_isaac.py:726-752).  Besides the weighted
 * total the four critic values are returned unweighted (the thesis compared critics by
 * commenting lines :325-329 in and out), and the number of waypoints in collision. */
enum mppi_cost_term {
  MPPI_TERM_PATH = 0, MPPI_TERM_SLOPE = 1, MPPI_TERM_SPEED = 2, MPPI_TERM_OBSTACLE = 3,
  MPPI_TERM_ORIENTATION = 4 /* mppi_get_cost_terms5 only */
};
typedef struct mppi_path_scores { /* host pointers, any may be NULL */
  float* cost;         /* [n]   weighted total, as costs_wp                                  */
  float* terms;        /* [n*4] unweighted critic values, mppi_cost_term order               */
  int32_t* collisions; /* [n]   waypoints with costmap > collision_threshold                 */
} mppi_path_scores;

/* Scores n paths of up to `stride` waypoints, trajectory-major like the dump arrays (host memory,
 * copied in and out): traj, left_wheel, right_wheel [n*stride*3], lin_vel [n*stride]; lengths [n]
 * (each in [1, stride]; NULL: every path has stride waypoints; rows past a path's length are not
 * read).  left_wheel and right_wheel are both given or both NULL; with NULL the slope critic runs
 * on the body path (_avoid_slope, critics_warp.py:131-166: the wheel form with both wheels on
 * traj).  origin: the robot position and goal the critics measure from (x, y, goal_x, goal_y; the
 * other fields are not read), NULL = the context's current state.  Weights, horizon (it does not
 * depend on stride), thresholds and v_max_linear are the context's params, the costmap the
 * context's.  Needs a costmap (MPPI_ESTATE otherwise), no DEM.  n * stride < 2^31.  Synchronous;
 * changes no state of the context.  The context's critic set applies: in MPPI_SLOPE_BODY the slope
 * critic reads traj even when wheel arrays are given, and with w_orientation != 0 `cost` has the
 * orientation term in front (robot = origin's x, y); `terms` stays [n*4]. */
int mppi_score_paths(mppi_ctx* ctx, int64_t n, int32_t stride, const int32_t* lengths,
                     const float* traj, const float* left_wheel, const float* right_wheel,
                     const float* lin_vel, const mppi_state* origin, mppi_path_scores* out);
/* The critic terms [K*4] and collision counts [K] of the last step's K rollouts of this context
 * (either may be NULL): re-runs the step like mppi_dump_rollouts with the dump buffers kept on
 * the device, scores them there and copies out 20 bytes per trajectory.  terms recombined as
 * critics_warp.py:325-329 (w_path * path, += w_slope * slope, += w_speed * speed,
 * += w_obstacle * obstacle) are the bits of mppi_get_costs whenever the critic set's w_orientation
 * is 0.  Term 1 is the slope value of the mode in force. */
int mppi_get_cost_terms(mppi_ctx* ctx, float* terms, int32_t* collisions);
/* The same with the orientation critic's value as a fifth term, [K*5] in mppi_cost_term order:
 * recombined in the order of the critic set's section (the orientation line first, only when its
 * weight is not 0) they are the bits of mppi_get_costs for any set. */
int mppi_get_cost_terms5(mppi_ctx* ctx, float* terms5, int32_t* collisions);
/* HIP-event time of the last scoring kernel of the context, in milliseconds. */
int mppi_get_score_ms(mppi_ctx* ctx, double* ms);

/* ---- batched closed-loop episodes ----
 * MPPI_Controller.run (MPPI_isaac.py:755-806) for E independent episodes at once, the loop's state
 * feedback done on the GPU: the closed-loop campaigns of the thesis (about 2 000 runs of up to 3 500
 * steps) and parameter sweeps.  The episodes share the context's parameters and, unless they hold
 * a variant, a scene slot or a trajectory count of their own (below), its scene (DEM, costmap) and
 * K; each has its own start pose, goal, sigmas and Philox seed.  Per step and batch three
 * launches on the context stream (normals, rollout, finish-and-advance), no host work in between.
 *
 * The advance rule after a step (float32 unless noted; v, w = element 0 of the filtered optimal
 * velocities, row 0 of the optimal rollout, r = params.robot_radius):
 *   x, y = traj_sim[0]; heading = heading_sim[0] in float64 / sqrt((h0 h0 + h1 h1) + h2 h2), each
 *   component rounded to float32; ww = (w w) / sigma_div; std_dev_u1 = max(sigma_base, sigma_base -
 *   ww); std_dev_u2 = max(sigma_base, sigma_base + ww); half = (w r) / 2; left_wheel_speed = v -
 *   half; right_wheel_speed = v + half; the goal is unchanged.
 * An episode is active before a step unless |x - goal_x| <= goal_tol and |y - goal_y| <= goal_tol (with
 * finite coordinates: iff |x - goal_x| > goal_tol or |y - goal_y| > goal_tol; a NaN coordinate is
 * never inside the tolerance, so a pose that is not a number does not count as reached).
 * {0.4, 1, 0.5} is run()'s policy (:763-784), {0.25, 3, 0.5} the Isaac loop's
 * (visual_terrain_stack_full_terrain.py:510-511).  Each step is bitwise the mppi_step of a context
 * with the episode's seed, state and step index. */
typedef struct mppi_batch mppi_batch;
typedef struct mppi_loop_policy {
  float sigma_base, sigma_div, goal_tol;
  int32_t check_every;   /* steps enqueued between host looks at the active count; 0 = 16 */
} mppi_loop_policy;
/* 1 <= episodes <= 4096; the context's K must give 1 to 16 leaf records of 256 trajectories
 * (K <= 4096; MPPI_EINVAL otherwise).  The batch borrows the context's scene and parameters at
 * every run (a DEM or costmap changed between runs is picked up); the context outlives the batch. */
int  mppi_batch_create(mppi_ctx* ctx, int32_t episodes, mppi_batch** out);
void mppi_batch_destroy(mppi_batch* b);
/* Episode e starts at `start` (heading used as given, as mppi_set_state) with Philox key `seed`,
 * a zero nominal sequence and step index 0, and is runnable; an episode never set does not run. */
int  mppi_batch_set_episode(mppi_batch* b, int32_t e, const mppi_state* start, uint64_t seed);
/* Stops the context's resident server, then advances every active episode by up to n_steps steps,
 * enqueued in chunks of policy->check_every; after each chunk the host waits and reads the count of
 * active episodes, and stops at 0.  Results do not depend on check_every.  A further call
 * continues every unfinished episode (the step index keeps counting); the log holds the rows of
 * the most recent run.  MPPI_ESTATE without a DEM and costmap, or after a HIP error of the batch. */
int  mppi_batch_run(mppi_batch* b, int32_t proj, int32_t n_steps, const mppi_loop_policy* policy);
/* Any output may be NULL.  state: the episode's current state; steps_total: steps since
 * set_episode; steps_last_run: steps of the most recent run; reached: the goal test has passed;
 * u1, u2 [H]: the nominal sequence the next step would read. */
int  mppi_batch_get_episode(mppi_batch* b, int32_t e, mppi_state* state, int64_t* steps_total,
                            int32_t* steps_last_run, int32_t* reached, float* u1, float* u2);
/* rows [count * 8]: x, y, z, the normalised heading, v, w of steps first .. first + count - 1 of the
 * most recent run (first + count <= steps_last_run). */
int  mppi_batch_get_log(mppi_batch* b, int32_t e, int32_t first, int32_t count, float* rows);
int  mppi_batch_get_ms(mppi_batch* b, double* ms);  /* HIP-event time of the last run */

/* ---- per-episode parameter variants ----
 * The thesis's campaigns vary "weights in the cost function, various terrain constraints, various
 * number of trajectories" (work summarise:52) and alternate a 2D and a 3D run of one task
 * (evaluate_trajectory.py:80-126).  A variant is the set of parameters that one batch can vary per
 * episode: plain kernel scalars that enter no plan, LDS size or shape.  The scene and the number
 * of trajectories are per episode too, through the batch's slots (next section).  Everything else
 * (num_iterations, dt, the control and velocity limits, wheel_offset, robot_radius, horizon,
 * goal_tol, check_every) stays the context's and the run's. */
typedef struct mppi_batch_variant {      /* 56 bytes */
  float w_path, w_slope, w_speed, w_obstacle;       /* critics_warp.py:325-329 */
  float collision_threshold, collision_penalty;     /* :251-253 */
  float temperature;
  float filter_k, filter_a, opt_filter_k, opt_filter_a;
  float sigma_base, sigma_div;                      /* the loop policy's sigma schedule */
  int32_t proj;                                     /* MPPI_PROJ_2D / MPPI_PROJ_3D */
} mppi_batch_variant;
/* out = the context's params with the given projection and the policy's sigma schedule: a variant
 * that changes nothing against mppi_batch_run(b, proj, n, policy). */
int  mppi_batch_variant_default(mppi_batch* b, int32_t proj, const mppi_loop_policy* policy,
                                mppi_batch_variant* out);
/* The batch's variant table: 0 <= n <= 1024 rows, copied to device memory; n = 0 clears it.  Each row
 * passes the range checks of mppi_create (temperature > 0) and needs sigma_div != 0 and proj in
 * {2, 3}; MPPI_EINVAL names the row and the field, and also answers a table shorter than an index an
 * episode holds.  Synchronous, like every batch call. */
int  mppi_batch_set_variants(mppi_batch* b, int32_t n, const mppi_batch_variant* v);
/* Episode e runs with row `variant` of the table; -1 (the default of every episode) = the
 * context's params and mppi_batch_run's proj / policy.  The index outlives mppi_batch_set_episode.
 * For an episode that holds a variant mppi_batch_run's proj and policy->sigma_base / sigma_div are
 * ignored; every step is bitwise the mppi_step of a context created with the batch context's
 * params overridden by the variant, with the variant's projection, advanced by the rule above with
 * the variant's sigma schedule.  Per step the rollout is launched once per projection in use. */
int  mppi_batch_set_episode_variant(mppi_batch* b, int32_t e, int32_t variant);
/* The critic sets of the variant rows: 0 <= n <= 1024 rows, copied to device memory; n = 0 clears
 * them.  Variant row i runs with critic row i if i < n; every other variant, and every episode or
 * task without a variant, runs with the context's set (mppi_set_critics).  Every step of such an
 * episode, task or device step is bitwise the mppi_step of a context with the variant's params
 * after mppi_set_critics(row).  MPPI_EINVAL names the row and the field (the checks of
 * mppi_set_critics).  The log scorers (mppi_batch_score, _score_tasks) use the context's set: a log
 * has no wheel arrays, so their slope critic is the body form in either mode. */
int  mppi_batch_set_variant_critics(mppi_batch* b, int32_t n, const mppi_critics* rows);
/* The sampling plans of the variant rows, by the rules of mppi_batch_set_variant_critics: variant row
 * i runs with plan row i if i < n; every other variant, and every episode or task without a variant,
 * runs with the context's plan (mppi_set_sampling) as it is at every run.  Applies to mppi_batch_run,
 * _run_tasks, _step_device and _step_tracked; every step of such an episode is bitwise the mppi_step of
 * a context after mppi_set_sampling(row).  MPPI_EINVAL names the row and the field. */
int  mppi_batch_set_variant_sampling(mppi_batch* b, int32_t n, const mppi_sampling* rows);

/* ---- per-episode scene and trajectory count ----
 * The campaign's other two axes: "various terrain constraints, various number of trajectories"
 * (a Monte-Carlo over rock fields, "when removing the rocks"; K = 1000 / 500 / 350).  A batch owns
 * up to 256 DEM slots (a copy of the heights and its normal table each) and 1024 costmap slots; an
 * episode may hold one of each and a trajectory count K_e, each independently of the others and of
 * its variant.  The defaults (-1, -1, 0) are the context's DEM, costmap and num_trajectories,
 * borrowed at every run as before.  Every step of an episode is bitwise the mppi_step of a context
 * created with the batch context's params (overridden by the episode's variant) with
 * num_trajectories = K_e and the same k_offset, after mppi_set_dem(Z of its slot) and
 * mppi_set_costmap(cm of its slot), with the episode's seed, state and step index; the Philox
 * address of a trajectory does not depend on K.
 * A slot takes the context's geometry at the time it is set (DEM: rows, cols, x_min, y_min,
 * resolution; costmap: size, half_width, resolution), so a DEM and a costmap must be set on the
 * context first (MPPI_ESTATE).  mppi_batch_run and mppi_batch_score return MPPI_ESTATE, naming the
 * slot, when an episode in use holds a slot whose geometry is no longer the context's.
 * z_host [rows * cols] / cm_host [size * size]: copied; setting a live slot again replaces its
 * contents; NULL frees the slot (MPPI_EINVAL while an episode holds it).  MPPI_EINVAL, naming the
 * slot, episode or field, for an index out of range, an episode given an empty slot and K_e outside
 * [1, the context's num_trajectories] (0 resets it).  A failed allocation is MPPI_EHIP with the
 * size; the slot and the batch stay as they were.  The scene and K_e of an episode outlive
 * mppi_batch_set_episode, as its variant index does.  All synchronous. */
int  mppi_batch_set_dem(mppi_batch* b, int32_t slot, const float* z_host);
int  mppi_batch_set_costmap(mppi_batch* b, int32_t slot, const float* cm_host);
/* mppi_build_costmap with the context costmap's size and half_width, straight into the slot
 * (out_host may be NULL).  MPPI_EINVAL if the context costmap's resolution is not
 * 2 * half_width / size, the builder's own. */
int  mppi_batch_build_costmap(mppi_batch* b, int32_t slot, const double* obstacles, int32_t n,
                              double origin_x, double origin_y, double r_robot, int32_t power,
                              int32_t metric, float* out_host);
/* mppi_batch_build_costmap with the steep cells of a DEM (mppi_build_costmap_hazard): dem_slot names
 * the batch's DEM slot whose heights are read in place (-1: the context's DEM), so a crater field
 * built into a slot (mppi_batch_build_dem) and its matching costmap never leave the device.
 * hz == NULL is exactly mppi_batch_build_costmap (dem_slot is then not looked at).  MPPI_ESTATE
 * when the DEM slot is empty or no DEM is bound; MPPI_EINVAL for a dem_slot outside the table.
 * out_host and mask_host may be NULL. */
int  mppi_batch_build_costmap_hazard(mppi_batch* b, int32_t slot, int32_t dem_slot, const double* obstacles,
                                     int32_t n, double origin_x, double origin_y, double r_robot,
                                     int32_t power, int32_t metric, const mppi_hazard* hz, float* out_host,
                                     uint8_t* mask_host);
/* mppi_build_dem into DEM slot `slot`, with the context DEM's geometry: the context's DEM must be square
 * with x_min = y_min = -(float)half_width and resolution (float)(2*half_width/rows) (MPPI_EINVAL
 * otherwise); MPPI_ESTATE without a context DEM.  Everything else as mppi_batch_set_dem (replacing a
 * live slot, an allocation failure leaves slot and batch as they were).  out_host may be NULL. */
int  mppi_batch_build_dem(mppi_batch* b, int32_t slot, const double* craters, int32_t n, double half_width,
                          const float* base_host, float* out_host, int32_t variant);
int  mppi_batch_set_episode_scene(mppi_batch* b, int32_t e, int32_t dem_slot, int32_t costmap_slot);
int  mppi_batch_set_episode_trajectories(mppi_batch* b, int32_t e, int64_t num_trajectories);

/* Scores every episode's executed path with one common cost function, on the device
 * (evaluate_trajectory.py:80-126 re-scores each logged run so).  The path of episode e is the log of
 * its most recent run: rows 0 .. steps_last_run-1, waypoint = (x, y, z), lin_vel = v; no wheel
 * arrays, so the slope critic runs on the body path, as mppi_score_paths with NULL wheels.  Each
 * path is scored on its episode's costmap: its costmap slot's, or the context's.
 * yardstick: the weights, collision_threshold and collision_penalty every path is scored with (its
 * other fields are not read); NULL = the context's params.  origins: NULL or [E] states of which x,
 * y, goal_x, goal_y are read; NULL = the episode's position when its most recent run began and the
 * episode's goal.  out: arrays of E (any may be NULL); rows [E] (may be NULL) receives each path's
 * length.  An episode with no rows gets cost 0, terms 0, collisions 0.  The log stays on the
 * device: 24 bytes per episode cross the bus.  mppi_get_score_ms of the batch's context reports the
 * kernel's HIP-event time.  Synchronous; changes no state. */
int  mppi_batch_score(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                      mppi_path_scores* out, int32_t* rows);

/* ---- a batch's task queue: N tasks on the batch's E episodes as lanes ----
 * A campaign is many runs of very different lengths (goal reached early, a detour, the step cap).
 * Run as plain batches, every episode that has ended idles until the slowest one of its batch ends,
 * and every batch costs E mppi_batch_set_episode calls and readbacks.  With a task list the lane
 * whose task ends takes the next task of the list itself, on the device, in the same step, until
 * the list is empty: no host work and no idle lane in between.
 * Contract, per task: every step is bitwise the mppi_step of a context with that task's seed, state,
 * step index (from 0), variant, DEM, costmap and num_trajectories, exactly as for an episode given
 * the same through the per-episode setters.  Which lane runs which task shows in no result.
 * A task whose start lies inside the goal tolerance takes no step: steps = 0, reached = 1. */
typedef struct mppi_batch_task {         /* 88 bytes */
  mppi_state start;                      /* the heading used as given */
  uint64_t   seed;                       /* Philox key */
  int32_t    variant;                    /* row of the batch's variant table, -1: none */
  int32_t    dem_slot, costmap_slot;     /* -1: the context's */
  int64_t    num_trajectories;           /* in [1, context K], 0: the context's */
  int32_t    max_steps;                  /* >= 1: the task ends unreached after this many steps */
} mppi_batch_task;
/* The batch's task list: n >= 1 tasks, copied to device memory, the results reset; n = 0 clears the
 * list.  Every task is checked by the rules of the per-episode setters (variant index inside the
 * table; slots live and of the context's current geometry; num_trajectories in [1, context K] or 0;
 * max_steps >= 1): MPPI_EINVAL names the task and the field, and the list stays as it was.  The log
 * arena of sum(max_steps) rows of 32 bytes is allocated here: MPPI_EHIP with the size when that
 * fails (the list is then empty).  While a list stands, a slot one of its tasks holds is not freed
 * and the variant table is not shortened below a row one of them names (MPPI_EINVAL, naming the
 * task).  Replacing or clearing the list of an unfinished campaign abandons it. */
int  mppi_batch_set_tasks(mppi_batch* b, int32_t n, const mppi_batch_task* tasks);
/* Advances the campaign by up to n_steps batch steps in chunks of policy->check_every, as
 * mppi_batch_run does, and stops early when every task has ended; a further call continues where
 * this one stopped.  The first call of a list fills the lanes (one claim launch).  proj and the
 * policy's sigma schedule apply to tasks without a variant, as for episodes; every call of one
 * campaign should pass the same.  tasks_done (may be NULL): tasks ended so far; batch_steps (may be
 * NULL): the batch steps of this call.  MPPI_ESTATE without a list, without a DEM and costmap, when
 * a listed slot no longer has the context's geometry, or after a HIP error of the batch.  When
 * every task has ended the call returns at once.
 * The episodes are the lanes: a campaign overwrites their states.  While a campaign is unfinished
 * mppi_batch_run answers MPPI_ESTATE.  When the campaign completes, or its list is replaced or
 * cleared, the episodes' own variant indices, scenes and trajectory counts are as before the
 * campaign, and every episode is un-set: not runnable until mppi_batch_set_episode. */
int  mppi_batch_run_tasks(mppi_batch* b, int32_t proj, int32_t n_steps, const mppi_loop_policy* policy,
                          int32_t* tasks_done, int64_t* batch_steps);
/* Task i's result (any output may be NULL): the state after its last step so far, the steps taken,
 * whether the goal test passed, and started = 0 (not yet claimed by a lane), 1 (running), 2 (ended). */
int  mppi_batch_get_task(mppi_batch* b, int32_t i, mppi_state* state, int32_t* steps, int32_t* reached,
                         int32_t* started);
/* Rows [first, first + count) of task i's log (8 floats each, as mppi_batch_get_log); MPPI_EINVAL
 * beyond the steps the task has taken. */
int  mppi_batch_get_task_log(mppi_batch* b, int32_t i, int32_t first, int32_t count, float* rows);
/* mppi_batch_score over the N task logs: each path on its task's costmap (its slot's, or the
 * context's).  origins: NULL or [N]; NULL = each task's start and goal.  out: arrays of N; rows [N].
 * A task that has not ended scores as a path without rows. */
int  mppi_batch_score_tasks(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                            mppi_path_scores* out, int32_t* rows);

/* ---- a scored task list: every task's score as it runs, with or without a log ----
 * Almost every campaign ends in mppi_batch_score_tasks with one yardstick, which needs the log arena
 * (32 bytes per step of every cap) and a second pass over it.  A list set scored is scored by the
 * lane that runs it: in the step that logs a row, the same lane extends the scorer's four critic
 * chains by that row, and when the task ends its score row is written beside its result.
 * Contract, per ended task i: cost, terms[4] (path, slope in the body form, speed, obstacle),
 * collisions and rows are bit for bit what mppi_batch_score_tasks(b, yardstick, NULL, ...) returns
 * for a logged run of the same list: origin = the task's start and goal, the task's own costmap
 * (its slot's, or the context's), the yardstick's weights, collision_threshold and
 * collision_penalty (its other fields are not read; NULL = the context's params), and the context's
 * w_orientation in front of the cost; the yardstick, w_orientation and v_max_linear are taken when
 * the list is set.  `length` is compute_length of evaluate_trajectory.py:43-53 on the task's
 * waypoints in float64: over the sampled rows 0, 5, 10, ... < rows, the sum in row order of
 * sqrt((dx dx + dy dy) + dz dz) between consecutive sampled rows, each difference of the float32
 * coordinates widened first; fewer than two sampled rows give 0.  A task that took no step, has
 * not ended or was not yet claimed has a row of zeros, as mppi_batch_score_tasks scores a path
 * without rows.
 * mppi_batch_set_tasks_scored is mppi_batch_set_tasks (the same checks and refusals, the same rules
 * about replacing or clearing a list; mppi_batch_run_tasks and mppi_batch_get_task as before) with
 * the yardstick and keep_log.  keep_log != 0: everything mppi_batch_set_tasks gives, and the scores.
 * keep_log = 0: no arena is allocated and no row is written, so the caps' sum has no limit and the
 * device holds 184 bytes per task (the task, its result, its score row) whatever the caps;
 * mppi_batch_get_task_log and mppi_batch_score_tasks then answer MPPI_ESTATE (the list keeps no
 * log). */
int  mppi_batch_set_tasks_scored(mppi_batch* b, int32_t n, const mppi_batch_task* tasks,
                                 const mppi_batch_variant* yardstick, int32_t keep_log);
/* The score rows of tasks [first, first + count): out's arrays of count (out, or any of its arrays,
 * may be NULL), rows [count] and length [count] (may be NULL).  One copy of count rows of 40 bytes,
 * no kernel launch.  MPPI_ESTATE when the standing list was not set scored; MPPI_EINVAL for a range
 * outside the list. */
int  mppi_batch_get_task_scores(mppi_batch* b, int32_t first, int32_t count, mppi_path_scores* out, int32_t* rows,
                                double* length);

/* ---- a batch's device-resident step: the plant is the caller's ----
 * mppi_batch_run feeds row 0 of the optimal rollout back as the next state: the plant is the
 * controller's own model.  The Isaac loop (visual_terrain_stack_full_terrain.py:466-515) hands
 * optimal_lin_vel_wp[0] / optimal_ang_vel_wp[0] to a simulator, reads the pose, heading and angular
 * velocity back from it and computes the sigmas from the measured angular velocity.  A vectorised
 * simulator of E rovers holds those in device memory; this call takes the states from there and
 * leaves the commands there, one step of every episode per call, with no host copy in between.
 * Asynchronous on the context's stream (the caller's after mppi_set_stream): the call enqueues the
 * launches (ingest, normals, one rollout per projection in use, finish) and returns, without a
 * stream wait, a host copy or a read of pinned memory.  It stops the context's resident server
 * first, as every batch call does: a host wait only while a server is running.  The arrays are read
 * and written in stream order; the caller keeps them alive until the step has run.  A HIP error of
 * an enqueued step surfaces at the next synchronous call of the batch (mppi_batch_get_episode,
 * _get_log, _run), which then refuses the batch as a failed run does (MPPI_ESTATE from then on).
 * Contract: for every set episode e that takes the step, cmd[e] and plan[e] are bitwise lin_vel[0],
 * ang_vel[0] and the listed outputs of mppi_step(ctx', proj_e, s_e), ctx' a context with the batch
 * context's params overridden by e's variant, num_trajectories = K_e, e's seed, DEM and costmap,
 * after mppi_set_state(states[e]) and with the nominal sequence e's previous step left (zero after
 * mppi_batch_set_episode or a reset); s_e = the steps e has taken since mppi_batch_set_episode or
 * its last reset.  Afterwards the new nominal sequence is the one the next step reads, s_e and
 * steps_total have grown by one, and e's record holds states[e] (what mppi_batch_get_episode
 * reports; `reached` reads 0: no goal test has seen that state).  No advance rule, no goal test, no
 * log row: steps_last_run and the log stay as the last mppi_batch_run left them.
 * An episode that is masked out or was never set does not step: its state, nominal sequence and
 * step index stay as they are and its rows of cmd and plan are not written.
 * proj applies to the episodes without a variant.  MPPI_EINVAL for a null io or null states;
 * MPPI_ESTATE without a DEM and costmap, while a campaign is unfinished, when a held slot's geometry
 * is no longer the context's, after a HIP error of the batch, and when the context does not run the
 * role-split plan.  May be mixed with mppi_batch_run, which continues from the record the last
 * device step left. */
typedef struct mppi_batch_io {   /* device pointers, on the batch context's device */
  const float*    states; /* [E][11] rows in mppi_state field order: x, y, heading[3],
                             left_wheel_speed, right_wheel_speed, goal_x, goal_y,
                             std_dev_u1, std_dev_u2; heading used as given (as mppi_set_state) */
  const int32_t*  mask;   /* [E] or NULL: episode e takes this step iff mask[e] != 0 (NULL: all set episodes) */
  const int32_t*  reset;  /* [E] or NULL: reset[e] != 0 restarts e before the step: zero nominal
                             sequence, step index 0, and seeds[e] as its Philox key if seeds != NULL */
  const uint64_t* seeds;  /* [E] or NULL; read only where reset[e] != 0 */
  float*          cmd;    /* [E][2] or NULL: v, w = element 0 of the filtered optimal velocities */
  float*          plan;   /* [E][4H+12] or NULL: u1_opt, u2_opt, lin_vel, ang_vel [H] each, then row 0 of
                             traj_sim, heading_sim, left_wheel_sim, right_wheel_sim */
} mppi_batch_io;
int  mppi_batch_step_device(mppi_batch* b, int32_t proj, const mppi_batch_io* io);

/* ---- tracked device steps: the run of an external plant, kept on the device ----
 * mppi_batch_step_device knows no run: a campaign in a simulator had to copy the states back every
 * frame to test the goal, keep the paths and upload them again for mppi_batch_score.  With tracking
 * set, every set episode carries a run that the ingest of mppi_batch_step_tracked logs, tests against
 * its goal and step cap, scores and ends, with no host copy and no synchronisation.
 * A run begins at mppi_batch_set_episode (with the first state ingested after it) or at a step with
 * reset[e] != 0; the state that begins it is its start and gives no row.  Every later ingest of the
 * run forms row n - 1 (n = 1, 2, ...) before anything else: x, y, z, heading[3] as given in
 * states[e], then v, w, the command the previous step of the episode wrote (the pose after the
 * command beside that command, as mppi_batch_run logs).  z is z_dev[e], the plant's pose height, or
 * with z_dev NULL the height of the episode's DEM (its slot's, or the context's) at (x, y) by the
 * rollout's lookup: the truncating cell index and the axis-swapped bilinear of projection_warp.py.
 * The row extends the run's score, and with keep_log it goes to the episode's log, where
 * mppi_batch_get_log and mppi_batch_score (origins NULL: the run's start and goal) read the current
 * or most recent run.  Then the goal test (|x - goal_x| <= goal_tol && |y - goal_y| <= goal_tol) on
 * the ingested state and the cap decide: the run ends reached, or unreached when its rows reach
 * max_steps.  A start inside the tolerance ends at once with steps 0, reached 1 and a score row of
 * zeros.  A reset that finds an unfinished run with at least one row ends it as abandoned (its state
 * and score are those of its last row); one without rows, and an unfinished run that
 * mppi_batch_set_episode replaces, leave no result.
 * The ending ingest writes the run's result into row r of the episode's result rows, r = the runs the
 * episode has ended since tracking was set, if r < runs_per_episode, and counts the run either way.
 * An ended episode does not step until its next reset: its rows of cmd and plan are not written and
 * its state, nominal sequence and step index stay.  done_dev [E] (may be NULL) receives, for every
 * set episode at every tracked step, 0 (running), 1 (reached) or 2 (the cap), and 0 for an episode
 * never set; the plant's own reset logic reads it in stream order.
 * The score row of a run is bit for bit what mppi_batch_score gives the same rows: cost, terms[4]
 * (path, slope in the body form, speed, obstacle), collisions and rows, with origin = the run's start
 * and goal, the episode's own costmap, the yardstick's weights, collision_threshold and
 * collision_penalty (NULL: the context's params) and the context's w_orientation; the yardstick,
 * w_orientation and v_max_linear are taken when tracking is set.  length: as mppi_batch_get_task_scores.
 * Every step that is taken keeps the contract of mppi_batch_step_device.
 * mppi_batch_set_tracking: max_steps >= 1 and runs_per_episode >= 1 turn tracking on (again: every run
 * and count starts over) and allocate 136 bytes per episode and 96 per result row, and with
 * keep_log != 0 max_steps log rows per episode (the log of an earlier mppi_batch_run is dropped);
 * max_steps = 0 turns it off and frees them.  goal_tol: the goal test's tolerance (the untracked step
 * takes no policy).  MPPI_EINVAL names the field; MPPI_ESTATE while a campaign is unfinished;
 * MPPI_EHIP with the sizes when the allocation fails (tracking is then off).  While tracking is set
 * mppi_batch_run, _set_tasks and _run_tasks answer MPPI_ESTATE: they write the same log and records.
 * Synchronous. */
int  mppi_batch_set_tracking(mppi_batch* b, const mppi_batch_variant* yardstick, float goal_tol, int32_t max_steps,
                             int32_t runs_per_episode, int32_t keep_log);
/* mppi_batch_step_device with the runs above: asynchronous in the same way, the same refusals, and
 * MPPI_ESTATE without tracking set.  z_dev [E] float and done_dev [E] int32: device pointers or NULL. */
int  mppi_batch_step_tracked(mppi_batch* b, int32_t proj, const mppi_batch_io* io, const float* z_dev,
                             int32_t* done_dev);
/* Result rows [first, first + count) of episode e (first + count <= runs_per_episode): the state at
 * the ending ingest, steps, reached, status (0: no run has ended into this row, 1: reached, 2: the
 * cap, 3: abandoned) and the score row (out's arrays of count, rows, length); any output may be NULL.
 * One copy of count rows of 96 bytes, no kernel launch.  Synchronous.  MPPI_ESTATE without tracking. */
int  mppi_batch_get_runs(mppi_batch* b, int32_t e, int32_t first, int32_t count, mppi_state* states, int32_t* steps,
                         int32_t* reached, int32_t* status, mppi_path_scores* out, int32_t* rows, double* length);
/* counts [E]: the runs each episode has ended since tracking was set; a count above runs_per_episode
 * says that results were dropped.  One copy, no kernel launch.  Synchronous. */
int  mppi_batch_get_run_counts(mppi_batch* b, int32_t* counts);

/* HIP-event timing of the rollout kernel and of the combine/optimal-rollout
 * kernel, measured on the context stream around each launch.  enable: 0 off,
 * 1 rollout, finish and deferred-tail events (the host waits for the stream and
 * for each tail to collect them), 2 rollout events only (no host wait; the finish
 * time reads 0).  In both modes each rollout launch waits for the work already on
 * the side streams, so no noise or deferred-tail kernel runs beside it: the
 * kernel's own time.  While timing is on,
 * steps run as separate launches (rollout, finish, tail), not on the resident
 * server, whose per-step kernel time no launch event brackets. */
int mppi_set_timing(mppi_ctx* ctx, int32_t enable);

/* Per-context options and test hooks, by name (MPPI_EINVAL for an unknown name):
 *   "resident"           sampled steps of the role-split plan (K <= 256 x CUs, records that fit
 *                        the in-kernel finish: C1-C3) on the resident step server, one launch that
 *                        stays on the GPU across steps and polls a command block in pinned memory
 *                        (mppi_step_server_kernel): no launch and no kernel boundary on a step's
 *                        path.  1 (default): for back-to-back calls only, i.e. a call within half
 *                        "resident_idle_us" of the last step's return keeps or starts it, and a
 *                        call after a longer gap (a simulator's frame: VERDICT r05 item 3, the
 *                        server's launch per frame cost more than the launches it saves) runs as
 *                        separate launches (launch_info[17]) and lets a running server go; 2: every
 *                        step whose plan fits; 0: never (env MPPI_RESIDENT=0/1/2 sets the default).
 *                        The server leaves after "resident_idle_us" without a step (a step posted
 *                        as it leaves is served by a relaunch, launch_info[15]), and every call on
 *                        the context other than mppi_step / mppi_set_state / mppi_get_outputs /
 *                        mppi_get_timing stops it first.  While it is resident it holds one
 *                        workgroup slot and ~154 KB of LDS on every CU: other kernels on the device
 *                        get the rest of each CU.  Results are bitwise those of separate launches.
 *   "resident_idle_us"   the server's idle limit, microseconds (default 200, [100, 1e6]).
 *   "finish_wait_ticks"  bound, in ticks of the 100 MHz s_memrealtime clock, on how long a
 *                        finish workgroup of the server waits for the step's rollout records
 *                        (default 1e5 = 1 ms: a running server's records arrive within microseconds
 *                        of each other; a fresh launch beside another stream's kernels that hold some
 *                        CUs has workgroups that cannot start).  A finish that gives up publishes
 *                        the failure; the host stops the server, waits for it to retire, re-arms
 *                        its counters and runs the step again as separate launches (same
 *                        results, launch_info[16]; 0: give up at once, the test hook).  A server
 *                        that does not retire within 10 s of its stop fails the call (MPPI_EHIP).
 *   "eps_after"          where separate launches and partial steps order the next steps' normals
 *                        (noise kernel, side stream): -1 (default) by the call's cadence, after the
 *                        finish for a call more than half "resident_idle_us" after the last step
 *                        returned (no event marker between the rollout and the finish: ~5 us less
 *                        latency per frame) and after the rollout for back-to-back calls and partial
 *                        steps (the noise then ends before the next rollout); 0 / 1: always after the
 *                        rollout / the finish.  Results are the same bits either way.
 *   "record_tree_finish" 1: the record-tree finish (mppi_finish_kernel) at every record count
 *                        (default 0: the column-split finish wherever its shape fits).
 *   "verified_reciprocal" test hook: 0 makes every cell index of the DEM and the costmap take the
 *                        IEEE division (the kernels' arm for a resolution with no verified
 *                        reciprocal, which no resolution tried so far reaches): it applies to the
 *                        bound DEM and costmap and to every later mppi_set_dem* / mppi_set_costmap /
 *                        mppi_build_costmap; 1 (default) restores the verified reciprocals.  Results
 *                        are the same bits either way.
 *   "server_exit_after"  test hook: the next server launch leaves at its poll after serving this
 *                        many steps, whether or not the next step was posted (0: off, default);
 *                        that step is served by a relaunch. */
int mppi_set_option(mppi_ctx* ctx, const char* name, int64_t value);
int mppi_get_timing(mppi_ctx* ctx, double* rollout_ms, double* finish_ms, int64_t* launches);
/* HIP-event time of the deferred optimal-rollout kernels (side stream). */
int mppi_get_tail_timing(mppi_ctx* ctx, double* tail_ms, int64_t* launches);

/* Layout/launch facts for the last step (for tests and the bench):
 * info[0]=0 (reserved), [1]=rollout block threads, [2]=rollout blocks, [3]/[4]=cols/rows of
 * the DEM window the step's lanes can touch, [5]=rollout LDS bytes, [6]=finish kind (1 =
 * column-split mppi_colfin_kernel, 0 = record tree mppi_finish_kernel), [7]=records padded
 * (column-split) or records (tree), [8]=columns per finish workgroup, [9]=finish workgroups,
 * [10]=steps whose sampled controls the rollout keeps in LDS, [11]=1 if the step ran on the
 * resident step server (mppi_step_server_kernel), else 0 (always 0 under a sampling plan with
 * beta > 0, whose steps are separate launches); [12]/[13]/[14] = server launches /
 * steps served / failed steps so far (mppi_set_option "resident"); [15] = commands posted to a
 * server that was leaving on its idle limit and served by a relaunch (included in [12]); [16] =
 * failed server steps rerun as separate launches; [17] = steps the server could have run that ran as
 * separate launches because the call was not back-to-back ("resident" 1); [18] = which cell
 * indices the next launch divides by a verified reciprocal: 1 the bound DEM's, 2 the bound
 * costmap's, 3 both, 0 neither (the IEEE division; mppi_set_option "verified_reciprocal").
 * Up to 19 values. */
int mppi_get_launch_info(mppi_ctx* ctx, int64_t* info, int32_t n);

/* Shader clock of the last sampled 3D rollout, from the chain wave of trajectories 0..63
 * (s_memtime / s_memrealtime at the start and the end of its H steps), up to 10 values:
 * out[0] = shader clock in MHz, [1] = shader cycles per chain step, [2] = the chain's
 * microseconds, [3] = its shader cycles; role-split kernel, workgroup 0, microseconds:
 * [4] = workgroup start -> chain start, [5] = chain end -> every role done, [6] -> leaf
 * record written; over all workgroups (the first 4096): [7] = first -> last workgroup start,
 * [8] = first -> last record written, [9] = first start -> last record (0 where not measured);
 * out[10 + b] = first start -> workgroup b's record.  Waits for the context stream. */
int mppi_get_chain_clock(mppi_ctx* ctx, double* out, int32_t n);

/* The resident step server's own clock (s_memrealtime, 100 MHz), summed over the steps it has
 * served since mppi_create: roll_us = command seen -> last rollout ticket (the rollout of all
 * workgroups, on the server), step_us = command seen -> completion word; steps = the steps summed.
 * Does not stop the server. */
int mppi_get_server_time(mppi_ctx* ctx, double* roll_us, double* step_us, int64_t* steps);

/* Standalone DEM bilinear kernel: for n query points
 * (x[i], y[i]) in device memory, heights[i] = corner lookup + bilinear exactly
 * as projection_warp.py:8-100, on the context's DEM. */
int mppi_bilinear_query(mppi_ctx* ctx, const float* x_dev, const float* y_dev, float* h_dev,
                        int64_t n);

/* LDS-tiled DEM lookup (projection_warp.py:8-100 per query).
 * mppi_bin_queries reorders n < 2^31 device-resident query points by 128x128-cell
 * DEM tile: xs_out/ys_out [n] tile by tile, perm[pos] = input index (int32) of the
 * point now at pos, tile_off [ntiles+1] (ntiles from mppi_bilinear_tiles);
 * synchronous (order inside a tile is unspecified).  mppi_bilinear_tiled then
 * computes h[pos] for the binned points, each tile's window staged once in LDS; it
 * is ASYNCHRONOUS on the context stream (mppi_sync waits).  Results are bitwise
 * identical to mppi_bilinear_query. */
int mppi_bilinear_tiles(mppi_ctx* ctx, int32_t* ntiles);
int mppi_bin_queries(mppi_ctx* ctx, const float* x_dev, const float* y_dev, int64_t n, float* xs_out_dev,
                     float* ys_out_dev, int32_t* perm_dev, int32_t* tile_off_dev);
int mppi_bilinear_tiled(mppi_ctx* ctx, const float* xs_dev, const float* ys_dev,
                        const int32_t* tile_off_dev, float* h_dev);
/* Wait for all work enqueued on the context stream. */
int mppi_sync(mppi_ctx* ctx);

/* Test hook: enqueue on `stream` (a hipStream_t of `device`; NULL = its null stream) `groups`
 * workgroups that each hold lds_bytes (<= 160 KiB) of a CU's LDS for `microseconds` (<= 1 s) and do
 * nothing else: another stream's kernels occupying CUs when a step is posted (the simulator's, in
 * the reference's loop, visual_terrain_stack_full_terrain.py:466-541).  Asynchronous. */
int mppi_debug_hold(int32_t device, void* stream, int32_t groups, int32_t lds_bytes, int32_t microseconds);

/* ---- reference-integrator mode "python25d"  ----
 * generate_trajectory_25D of thesis_master/python_mppi_projection/debug.py:312-364,
 * the reference's numpy 2.5D integrator, for n trajectories at once, in float64,
 * on the context's DEM (row j at y = linspace(-half_width, half_width, rows)[j],
 * as debug.py's meshgrid; `resolution` as its `resolution` argument).  Inputs
 * (host): x0, y0 [n], heading [n*3], lin_vel, ang_vel [n*H] trajectory-major;
 * outputs (host): traj [n*H*3] (x, y, height per step), valid [n] (0 where the
 * reference returns None: the trajectory left |x|, |y| < bound, debug.py:359;
 * its rows from that step on are 0).  Synchronous.  Not on the MPPI step path:
 * it lets whole trajectories be compared with the reference's own function. */
int mppi_rollout_python25d(mppi_ctx* ctx, int64_t n, int32_t H, const double* x0, const double* y0,
                           const double* heading, const double* lin_vel, const double* ang_vel,
                           double dt, double half_width, double resolution, double bound,
                           double* traj, int32_t* valid);

/* Device self-test of the engine's exact-arithmetic fast paths: what = 0 checks
 * the shared-reciprocal division against IEEE a/b, what = 1 the sqrt path
 * against IEEE sqrtf, what = 2 / 3 the lean normalisation of the pair kernel's
 * chain (sqrt of a squared norm and three quotients; 3 with one dominant
 * component) against IEEE sqrtf and a/b, on n random operands; what = 4 the
 * chain's quotient (refined reciprocal, one residual correction) against a/b
 * for every significand of a and n / 2^23 divisor significands ((seed + 8191 k)
 * mod 2^23); what = 5 the noise radius' square root (sqrt_bm) against sqrtf
 * for -0, +0 and the n - 2 floats from 2^-24 up (n <= 2 + 0x4C000000); what = 6
 * the chain's normalisation of a vector that is already unit (square root and
 * reciprocal without a transcendental, three quotients) against sqrtf and a/b for
 * the squared norms (i >> 18) - 4096 ulps from 1, i < n <= 8193 * 2^18, with 2^18
 * numerator triples each (zeros and both signs among them): a norm beyond 2047
 * ulps must come back flagged for the IEEE redo and counts as a mismatch if it
 * does not; *mismatches receives the count of in-range results that differ in
 * any bit (0 expected). */
int mppi_selftest(mppi_ctx* ctx, int32_t what, int64_t n, uint64_t seed, int64_t* mismatches);

/* ---- Executed paths: wheel contacts, the wheel form of the slope critic, path metrics ----
 *
 * A log row holds x, y, z, heading, v, w.  The three options below add what the controller itself
 * steers by and what the 2D-vs-3D comparison quotes per run.  All are opt-in: a batch that calls none
 * of these entry points allocates, launches and computes what it did without them.
 *
 * The wheel log.  mppi_batch_set_wheel_log(b, 1): runs (mppi_batch_run), task lists (mppi_batch_set_tasks,
 * _set_tasks_scored with keep_log) and tracking (mppi_batch_set_tracking with keep_log) that are set
 * afterwards keep, beside every log row, the row's wheel contacts lx, ly, lz, rx, ry, rz: 24 bytes per
 * row in an array parallel to the log; the 8-float log row and its getters do not change.  Own model:
 * row n's contacts are row 0 of left_wheel_sim / right_wheel_sim of that step's optimal rollout (floats
 * 4H + 6 .. 4H + 11 of the plan), the bits of the single-context mppi_step, whichever projection planned.
 * Tracked steps: the ingest forms them from the ingested pose by the rollout's rule
 * (projection_warp.py:331-347): q = the corners of the cell of (x, y) on the episode's DEM,
 * n = normal_on_grid(q), c = cross(n, heading as given), r = wheel_offset (c.x, c.y), left =
 * (x + r.x, y + r.y, Z[cell(x + r.x, y + r.y)]), right the same with -r; IEEE float32 / and sqrt.
 * MPPI_ESTATE while a campaign is unfinished or tracking is set.  The getters mirror mppi_batch_get_log
 * and mppi_batch_get_task_log (rows6: count * 6 floats); MPPI_ESTATE when the log has no wheel log. */
int mppi_batch_set_wheel_log(mppi_batch* b, int32_t enable);
int mppi_batch_get_wheel_log(mppi_batch* b, int32_t e, int32_t first, int32_t count, float* rows6);
int mppi_batch_get_task_wheel_log(mppi_batch* b, int32_t i, int32_t first, int32_t count, float* rows6);

/* compute_path_metrics of the reference (MPPI_isaac.py:231-256, k = 20) of one executed path, float64.
 * Waypoints: the rows' float32 (x, y, z) widened.  Segments m = 0, 1, ... while 20 m + 21 < rows:
 * s = p[20 m + 21] - p[20 m]; hh = s.x s.x + s.y s.y; n = sqrt(hh + s.z s.z); length20 += n; if n > 0:
 * a = dm_atan2(s.z, sqrt(hh)) (180 / pi), a > 0 adds a to angle_up, else |a| to angle_down; if s.z > 0:
 * distance_up += s.z.  Sums in row order, no fused operation; fewer than 22 rows give zeros.  dm_atan2 is
 * the deterministic arctangent of csrc/mppi_detmath.h; mppi_amd.batch.path_metrics is the numpy form. */
typedef struct mppi_path_metrics {
  double length20, angle_up, angle_down, distance_up;
} mppi_path_metrics;

/* mppi_batch_score / mppi_batch_score_tasks with a choice of the slope term and the path metrics.
 * slope_mode MPPI_SLOPE_BODY: the existing entry points' results.  MPPI_SLOPE_WHEELS: the slope term
 * reads the wheel log's two contact paths: cost, terms, collisions and rows are bitwise those of
 * mppi_score_paths on a context in MPPI_SLOPE_WHEELS given the log's (x, y, z) as traj, the wheel log's
 * halves as left_wheel / right_wheel, the log's v and the same origin, yardstick and costmap;
 * MPPI_ESTATE, naming mppi_batch_set_wheel_log, when the log has no wheel log.  metrics: [E] ([N] for
 * tasks) rows or NULL. */
int mppi_batch_score_ex(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                        int32_t slope_mode, mppi_path_scores* out, int32_t* rows, mppi_path_metrics* metrics);
int mppi_batch_score_tasks_ex(mppi_batch* b, const mppi_batch_variant* yardstick, const mppi_state* origins,
                              int32_t slope_mode, mppi_path_scores* out, int32_t* rows,
                              mppi_path_metrics* metrics);

/* The same for the scores computed as the run goes: the next mppi_batch_set_tasks_scored or
 * mppi_batch_set_tracking takes slope_mode and metrics with its yardstick (default MPPI_SLOPE_BODY, 0).
 * In MPPI_SLOPE_WHEELS the advance lane (own model) or the ingest (tracked steps) extends the slope
 * chain over the row's wheel contacts; the score rows are bitwise mppi_batch_score_tasks_ex / _score_ex
 * on the same rows, with or without a log.  metrics != 0: a mppi_path_metrics row beside every score
 * row (zeros until the task or run ends).  MPPI_ESTATE while a campaign is unfinished or tracking is
 * set; the getters answer MPPI_ESTATE when the list or tracking was set without the metrics. */
int mppi_batch_set_score_options(mppi_batch* b, int32_t slope_mode, int32_t metrics);
int mppi_batch_get_task_metrics(mppi_batch* b, int32_t first, int32_t count, mppi_path_metrics* metrics);
int mppi_batch_get_run_metrics(mppi_batch* b, int32_t e, int32_t first, int32_t count,
                               mppi_path_metrics* metrics);

/* A read-out of the deterministic float64 arctangent on the device, for tests and measurements: for
 * the n pairs y[i], x[i] (host arrays, n <= 2^28) dm[i] = dm_atan2(y[i], x[i]) as the metrics' kernels
 * compute it (bitwise mppi_amd.batch.dm_atan2) and dev[i] = the device library's own atan2.  One small
 * kernel on the context's stream; synchronous; changes no state of the context. */
int mppi_detmath_atan2(mppi_ctx* ctx, int64_t n, const double* y, const double* x, double* dm, double* dev);

#ifdef __cplusplus
}
#endif

#endif /* HUSKY_MPPI_H */
