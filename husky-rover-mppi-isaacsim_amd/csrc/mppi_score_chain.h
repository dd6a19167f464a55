// The steps of the four critic chains of a scored path and their final combination, one statement
// of each rule (critics_warp.py:85-329; oracle/mppi_ref.py critics), float32 in the reference's order.
// Two callers: the path scorer (mppi_score.hip), which walks whole paths out of LDS, and the advance
// lane of the scored campaign finish (mppi_batch_kernels.h), which extends the same chains by one row
// per step.  Every chain is sequential in t, so both land on the same bits.
#pragma once

#include <hip/hip_runtime.h>

namespace mppi {
namespace chain {

// critics_warp.py:120-123, one waypoint's term of the near branch (the sum runs over t < L - 1)
__device__ __forceinline__ float path_near(float x, float y, float gx, float gy) {
  return 10.0f * (fabsf(x - gx) + fabsf(y - gy));
}

// critics_warp.py:111-119, the far branch: the terminal waypoint against the intermediate goal
__device__ __forceinline__ float path_far(float x, float y, float igx, float igy, float pf_scale) {
  const float dx = x - igx;
  const float dy = y - igy;
  return (dx * dx + dy * dy) * pf_scale;
}

// critics_warp.py:190-218: (1 + 5 |dz / (d + 1e-6)|)^2 between waypoints t and t + 2 of one wheel.
__device__ __forceinline__ float slope_one(const float (&p)[3], const float (&c)[3]) {
  const float dz = c[2] - p[2];
  const float dx = c[0] - p[0], dy = c[1] - p[1];
  const float d = sqrtf(dx * dx + dy * dy);
  const float ratio = fabsf(dz / (d + 1e-6f));
  const float s = 1.0f + 5.0f * ratio;
  return s * s;
}

// critics_warp.py:281-300, one waypoint (when speed_on)
__device__ __forceinline__ float speed(float acc, float vmax, float vt) { return acc + (vmax - vt) / (vt + 0.0001f); }

// critics_warp.py:244-248 (oracle costmap_at): clamp(trunc(clamp(f, -1, size)), 0, size - 1) is
// trunc(clamp(f, 0, size - 1)); a NaN coordinate indexes cell 0, as the oracle's fmax / fmin.
__device__ __forceinline__ int cm_index(float hw, float res_c, int cm_size, float x, float y) {
  const float fx = (x + hw) / res_c;
  const float fy = ((-y) + hw) / res_c;
  const float top = (float)(cm_size - 1);
  const int ix = (int)fminf(fmaxf(fx, 0.0f), top);
  const int iy = (int)fminf(fmaxf(fy, 0.0f), top);
  return ix + cm_size * iy;
}

// critics_warp.py:244-262, one waypoint whose costmap cell holds c: the penalty and the collision
// count before `+ c`.  (The pair goes in and out by value: with the count behind a reference the
// scorer's obstacle wave came out with two registers renamed.)
struct ObstacleAcc {
  float acc;
  int col;
};
__device__ __forceinline__ ObstacleAcc obstacle(float acc, int col, float c, float thr, float pen) {
  if (c > thr) {
    acc = acc + pen;
    ++col;
  }
  acc = acc + c;
  return ObstacleAcc{acc, col};
}

// critics_warp.py:44-82, as the rollout kernels' orientation_term: the origin (x0, y0), the goal and
// the path's last two waypoints (a path of one waypoint has no last displacement: the caller's 0)
__device__ __forceinline__ float orientation(float gx, float gy, float x0, float y0, float ex0, float ey0, float ex1,
                                             float ey1) {
  const float xd = gx - x0, yd = gy - y0;
  const float s = (xd * (ex1 - ex0)) + (yd * (ey1 - ey0));
  const float den = fabsf(xd) + fabsf(yd);
  return (s <= 0.0f && den != 0.0f) ? (-s) / den : 0.0f;
}

// critics_warp.py:324-329; the orientation term is the menu's first line, when it exists
__device__ __forceinline__ float combine(float w_path, float w_slope, float w_speed, float w_obs, float w_orient,
                                         float pf, float sw, float sp, float ob, float po) {
  float cost = w_path * pf;
  if (w_orient != 0.0f) cost = w_orient * po + cost;
  cost = cost + w_slope * sw;
  cost = cost + w_speed * sp;
  cost = cost + w_obs * ob;
  return cost;
}

}  // namespace chain
}  // namespace mppi
