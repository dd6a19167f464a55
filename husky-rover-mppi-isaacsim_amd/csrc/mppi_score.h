// Scoring of caller-supplied paths with the four critics of critics_warp.py:85-329
// (oracle/mppi_ref.py critics), see mppi_score.hip.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace mppi {

// The kernel's tile: SCORE_PATHS paths per 256-thread workgroup, staged SCORE_CHUNK waypoints at a time.
// Chunk 12 keeps the workgroup's LDS at 33 KB, four workgroups per CU: the 1024 workgroups of the
// step-shaped call (n = 65 536) are then one round on 256 CUs.  Measured at that shape: chunk 16
// (43 KB, three per CU, a second round one third full) 0.126 ms, 12: 0.090 ms, 8: 0.100 ms
// (profiles/score_paths.json).
constexpr int SCORE_PATHS = 64;
constexpr int SCORE_CHUNK = 12;
constexpr int SCORE_THREADS = 256;

// The goal terms of one path where every path has its own origin and goal (the episodes of a batch):
// state_fields() of mppi_capi.cpp, computed on the host.
struct ScoreGoal {
  float gx, gy, igx, igy, pf_scale;
  int pf_far, speed_on;
  float x0, y0;  // the origin: the orientation critic's robot position
  int pad;
};
static_assert(sizeof(ScoreGoal) == 40, "ScoreGoal layout");

struct ScoreArgs {
  // paths, trajectory-major (device memory)
  const float* traj;       // [n][stride][3]; with `log`: not read
  const float* lw;         // [n][stride][3] or null (then rw is null too: the slope critic reads traj)
  const float* rw;
  const float* v;          // [n][stride]
  const int32_t* lengths;  // [n], each in [1, stride], or null (every path has stride waypoints)
  // the log of a batch (mppi_batch_score) instead of traj / v: [n][stride][8] rows x, y, z, heading, v, w,
  // 32-byte aligned; then rw = null, lengths[p * len_step] (>= 0, clamped to stride) is path p's
  // length, goals [n] replaces gx .. speed_on below, and rows_out [n] (or null) receives the lengths;
  // lw is null, or the batch's wheel-contact log: rows of 6 floats (lx, ly, lz, rx, ry, rz) with the
  // log's own row index, which the slope critic then reads in place of the body path
  const float* log;
  const ScoreGoal* goals;
  int len_step;
  int32_t* rows_out;
  int64_t n;
  int stride;              // n * stride < 2^31
  // costmap (critics_warp.py:244-248)
  const float* cm;
  int cm_size;
  float hw, res_c;
  // goal terms precomputed in float32 in the reference's order (state_fields in mppi_capi.cpp)
  float gx, gy, igx, igy, pf_scale;
  int pf_far, speed_on;
  float vmax, thr, pen;
  float w_path, w_slope, w_speed, w_obs;
  // the orientation critic (mppi_critics::w_orientation; 0: the cost has no such term) and its robot
  // position, the origin (with `log`: goals[p].x0, y0).  The slope mode is the caller's choice of
  // lw / rw: null scores the body path.
  float w_orient, x0, y0;
  // outputs (device memory; any may be null)
  float* cost;          // [n]
  float* terms;         // [n][4] path, slope, speed, obstacle (16-byte aligned)
  int32_t* collisions;  // [n]
  float* orient;        // [n] the orientation critic's value (mppi_get_cost_terms5)
  // with `log` only: [n] each path's own costmap of cm's geometry (device pointers; an episode's
  // costmap slot, mppi_batch_score), or null: every path on cm
  const float* const* cm_path;
  // with `log` only: [n] the first row of each path in the log (device memory, rows >= 0: the task
  // logs of a batch, an arena of paths of different capacities; mppi_batch_score_tasks), or null:
  // path p begins at row p * stride.  With base rows `stride` only bounds the lengths.
  const int64_t* base_row;
};

hipError_t launch_score(const ScoreArgs& a, hipStream_t st);

// compute_path_metrics (mppi_path_metrics.h) of the n paths of a log ([.][8] rows; lengths, len_step,
// base_row (or null: path p begins at row p * stride) and stride as ScoreArgs has them) into out [n].
hipError_t launch_atan2_probe(const double* y, const double* x, int64_t n, double* dm, double* dev, hipStream_t st);
struct PathMetrics;
hipError_t launch_log_metrics(const float* log, const int32_t* lengths, int len_step, const int64_t* base_row,
                              int stride, int64_t n, PathMetrics* out, hipStream_t st);

}  // namespace mppi
