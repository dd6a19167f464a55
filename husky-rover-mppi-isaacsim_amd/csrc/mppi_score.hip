// Scoring of caller-supplied paths: the four critics of critics_warp.py:85-329 (oracle/mppi_ref.py
// critics) applied to paths the engine did not just roll out: logged closed-loop runs
// (evaluate_trajectory.py), the chosen plan (MPPI_isaac.py:726-752), or a step's own rollouts when the
// per-critic terms are wanted (mppi_get_cost_terms).  Every op is float32 in the reference's order;
// each critic's sum is one sequential chain in t (no reduction across t), so the values are the bits
// the rollout kernels' cost wave produces for the same points.
//
// Shape.  A path's row is stride * 12 bytes per array, so one lane per path reading global memory
// would touch a new cache line with every lane.  Instead a workgroup of 4 waves owns SCORE_PATHS = 64
// paths and walks them SCORE_CHUNK = 12 waypoints at a time:
//   load   all 256 threads run along the paths' contiguous floats (a chunk of one path is 144
//          contiguous bytes of traj / lw / rw and 48 of v), 16 bytes per lane when the rows are
//          16-byte aligned (stride % 4 == 0), else 4; the chunk after the one being scored is in
//          flight in registers while the critics run;
//   stage  the chunk goes to LDS as [path][3 * 12 + 1] (v: [path][12 + 1]) floats: the odd row
//          stride puts the 32 lanes of a ds_read_b32 group, which read the same waypoint of 32
//          different paths, on 32 different banks;
//   score  lane = path, wave = critic: wave 0 extends the path-follow chain, wave 1 the slope chain
//          (it carries the previous even waypoint across chunks), wave 2 the speed chain, wave 3 the
//          obstacle chain with its costmap gather and the collision count.  The four chains are
//          independent, so splitting them over waves keeps every chain's order and keeps all four
//          SIMDs busy with 64 paths per workgroup.
// The chunk loop runs to the longest path of the tile, whatever the stride: LDS use does not depend
// on the path length.  Rows past a path's length are staged but never enter a chain.
//
// LOG instantiation (mppi_batch_score): the paths are the rows of a batch's log, [path][stride][8]
// floats (x, y, z, heading, v, w), each path with its own goal terms (ScoreGoal).  A waypoint is one
// 32-byte row, so a thread takes whole waypoints: one aligned 16-byte load (x, y, z and a heading
// component it drops) and the 4 bytes of v, 3 waypoints per thread and chunk; a chunk of one path
// is 12 x 32 contiguous bytes and consecutive lanes read consecutive rows.  Only x, y, z, v are
// staged, into the same LDS rows (strides 37 and 13), so the score phase is the same code; pf_far
// and speed_on become per-lane branches.
//
// LOG with WHEELS (mppi_batch_score_ex, MPPI_SLOPE_WHEELS): the batch also kept a wheel-contact log,
// [row][6] floats (lx, ly, lz, rx, ry, rz) with the log's own row index (ScoreArgs::lw).  A thread takes
// the 24 bytes of its waypoints' contacts beside the row and stages them into the wheel arrays' LDS rows,
// so the slope wave is the caller-supplied paths' WHEELS code; the other three waves do not change.
//
// The path metrics of a log (mppi_log_metrics_kernel): compute_path_metrics of the reference in float64
// (mppi_path_metrics.h), one lane per path: a path of L rows has (L - 2) / 20 segments of two rows each,
// so a lane reads 64 bytes per 20 rows and the kernel is a handful of dependent loads per path.
#include "mppi_score.h"
#include "mppi_path_metrics.h"
#include "mppi_score_chain.h"

#include <algorithm>
#include <type_traits>

namespace mppi {

namespace {

constexpr int TP = SCORE_PATHS, CT = SCORE_CHUNK, NT = SCORE_THREADS;
constexpr int ROW3 = 3 * CT + 1;  // floats per path of a staged [t][3] chunk (odd: see above)
constexpr int ROWV = CT + 1;
static_assert(NT == 4 * 64 && TP == 64, "one wave per critic, one lane per path");
static_assert(CT % 4 == 0, "a chunk is whole 16-byte vectors of v and of the [t][3] arrays, and starts on an even t");

struct Smem {
  float a[3][TP * ROW3];  // traj, lw, rw
  float v[TP * ROWV];
  float term[4][TP];
  int col[TP];
};

// The registers that hold the chunk in flight: a thread's share of the tile's vectors of VEC floats
// (C floats per waypoint), rounded up to whole vectors.
constexpr int stage_floats(int C, int VEC) { return (TP * CT * C / VEC + NT - 1) / NT * VEC; }
template <int VEC>
struct Stage {
  float a[3][stage_floats(3, VEC)];
  float v[stage_floats(1, VEC)];
};

// One array's share of a chunk: C floats per waypoint, `len` waypoints from t0 of paths p0 .. p0 + TP - 1.
// Vector j of the tile = VEC floats at offset (j % spv) * VEC of path j / spv, spv = C * len / VEC.
template <int VEC, int C, int NF, bool STORE>
__device__ __forceinline__ void stage_array(const float* __restrict__ g, float (&r)[NF], float* s, int row,
                                            int64_t p0, int64_t n, int stride, int t0, int len, int tid) {
  constexpr int NV = NF / VEC;
  constexpr int SPV_FULL = C * CT / VEC;
  const bool full = len == CT;
  const int spv = full ? SPV_FULL : C * len / VEC;
  const int total = TP * spv;
#pragma unroll
  for (int i = 0; i < NV; ++i) {
    const int j = tid + i * NT;
    if (j >= total) continue;
    const int pp = full ? j / SPV_FULL : j / spv;
    const int o = (j - pp * spv) * VEC;
    if (p0 + pp >= n) continue;
    if constexpr (!STORE) {
      const float* src = g + ((size_t)(p0 + pp) * (size_t)stride + (size_t)t0) * C + o;
      if constexpr (VEC == 4) {
        const float4 q = *reinterpret_cast<const float4*>(src);
        r[4 * i] = q.x;
        r[4 * i + 1] = q.y;
        r[4 * i + 2] = q.z;
        r[4 * i + 3] = q.w;
      } else {
        r[i] = *src;
      }
    } else {
      float* dst = s + pp * row + o;
#pragma unroll
      for (int k = 0; k < VEC; ++k) dst[k] = r[VEC * i + k];
    }
  }
}

// LOG: the chunk in flight, x, y, z, v of the thread's waypoints.
constexpr int LOG_WP = TP * CT / NT;
static_assert(LOG_WP * NT == TP * CT, "whole waypoints per thread");
template <bool WHEELS>
struct StageLogT {
  float q[LOG_WP][WHEELS ? 10 : 4];  // x, y, z, v, then (WHEELS) the row's six contact floats
};
using StageLog = StageLogT<false>;

// Waypoint u of the tile = row t0 + u % len of path p0 + u / len.  RAGGED: path p begins at row
// base_row[p] of the log (an arena of paths of different capacities) instead of p * stride.
template <bool STORE, bool RAGGED, bool WHEELS>
__device__ __forceinline__ void stage_chunk_log(const ScoreArgs& a, StageLogT<WHEELS>& r, Smem& sm, int64_t p0, int t0,
                                                int len, int tid) {
  const bool full = len == CT;
  const int total = TP * len;
#pragma unroll
  for (int i = 0; i < LOG_WP; ++i) {
    const int u = tid + i * NT;
    if (u >= total) continue;
    const int pp = full ? u / CT : u / len;
    const int tt = u - pp * len;
    if (p0 + pp >= a.n) continue;
    if constexpr (!STORE) {
      size_t row;
      if constexpr (RAGGED)
        row = (size_t)a.base_row[p0 + pp] + (size_t)(t0 + tt);
      else
        row = (size_t)(p0 + pp) * (size_t)a.stride + (size_t)(t0 + tt);
      const float* src = a.log + row * 8;
      const float4 xyz = *reinterpret_cast<const float4*>(src);
      r.q[i][0] = xyz.x;
      r.q[i][1] = xyz.y;
      r.q[i][2] = xyz.z;
      r.q[i][3] = src[6];
      if constexpr (WHEELS) {  // a row of the wheel log is 24 bytes: 8-byte aligned
        const float2* w = reinterpret_cast<const float2*>(a.lw + row * 6);
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          const float2 c = w[k];
          r.q[i][4 + 2 * k] = c.x;
          r.q[i][5 + 2 * k] = c.y;
        }
      }
    } else {
      float* dst = sm.a[0] + pp * ROW3 + 3 * tt;
      dst[0] = r.q[i][0];
      dst[1] = r.q[i][1];
      dst[2] = r.q[i][2];
      sm.v[pp * ROWV + tt] = r.q[i][3];
      if constexpr (WHEELS) {
        float* dl = sm.a[1] + pp * ROW3 + 3 * tt;
        float* dr = sm.a[2] + pp * ROW3 + 3 * tt;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
          dl[k] = r.q[i][4 + k];
          dr[k] = r.q[i][7 + k];
        }
      }
    }
  }
}

template <int VEC, bool WHEELS, bool STORE, bool RAGGED>
__device__ __forceinline__ void stage_chunk(const ScoreArgs& a, StageLogT<WHEELS>& r, Smem& sm, int64_t p0, int t0,
                                            int len, int tid) {
  stage_chunk_log<STORE, RAGGED, WHEELS>(a, r, sm, p0, t0, len, tid);
}

template <int VEC, bool WHEELS, bool STORE, bool RAGGED>
__device__ __forceinline__ void stage_chunk(const ScoreArgs& a, Stage<VEC>& r, Smem& sm, int64_t p0, int t0, int len,
                                            int tid) {
  stage_array<VEC, 3, stage_floats(3, VEC), STORE>(a.traj, r.a[0], sm.a[0], ROW3, p0, a.n, a.stride, t0, len, tid);
  if constexpr (WHEELS) {
    stage_array<VEC, 3, stage_floats(3, VEC), STORE>(a.lw, r.a[1], sm.a[1], ROW3, p0, a.n, a.stride, t0, len, tid);
    stage_array<VEC, 3, stage_floats(3, VEC), STORE>(a.rw, r.a[2], sm.a[2], ROW3, p0, a.n, a.stride, t0, len, tid);
  }
  stage_array<VEC, 1, stage_floats(1, VEC), STORE>(a.v, r.v, sm.v, ROWV, p0, a.n, a.stride, t0, len, tid);
}

// The chains' steps are mppi_score_chain.h's: one statement of each rule, shared with the advance lane
// of the scored campaign (mppi_batch_kernels.h).
using chain::slope_one;

// LOG: the paths are a batch's log with per-path goal terms (see above); VEC = 1, WHEELS = false there.
// RAGGED (mppi_batch_score_tasks): the LOG loader with a base row per path (ScoreArgs::base_row).
template <int VEC, bool WHEELS, bool LOG = false, bool RAGGED = false>
__global__ __launch_bounds__(NT) void mppi_score_kernel(ScoreArgs a) {
  static_assert(!LOG || VEC == 1, "the log loader takes whole rows (WHEELS: and the rows of the wheel log)");
  static_assert(!RAGGED || LOG, "base rows belong to the log loader");
  __shared__ Smem sm;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int role = tid >> 6;  // wave-uniform: 0 path, 1 slope, 2 speed, 3 obstacle
  const int64_t p0 = (int64_t)blockIdx.x * TP;
  const int64_t p = p0 + lane;
  int L;
  if constexpr (LOG)
    L = p < a.n ? min(max(a.lengths[(size_t)p * a.len_step], 0), a.stride) : 0;
  else
    L = p < a.n ? (a.lengths ? min(a.lengths[p], a.stride) : a.stride) : 0;
  int Lmax = L;  // the tile's longest path: the same value in every wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) Lmax = max(Lmax, __shfl_xor(Lmax, o, 64));
  Lmax = min(Lmax, a.stride);
  // staged waypoints: whole 16-byte vectors (stride % 4 == 0 there, so still within the rows)
  const int Lld = VEC == 4 ? (Lmax + 3) & ~3 : Lmax;

  float acc = 0.0f;  // this wave's chain
  int col = 0;
  float pl[3] = {0.0f, 0.0f, 0.0f}, pr[3] = {0.0f, 0.0f, 0.0f};  // slope: the previous even waypoint
  float ex[2] = {0.0f, 0.0f}, ey[2] = {0.0f, 0.0f};  // path wave: waypoints L - 2 and L - 1 (the orientation critic)

  // the goal terms: kernel arguments, or (LOG) the lane's own path's, each wave loading its critic's
  float gx = a.gx, gy = a.gy, igx = a.igx, igy = a.igy, pf_scale = a.pf_scale, x0 = a.x0, y0 = a.y0;
  int pf_far = a.pf_far, speed_on = a.speed_on;
  if constexpr (LOG) {
    if (p < a.n) {
      const ScoreGoal* g = a.goals + p;
      if (role == 0) {
        gx = g->gx;
        gy = g->gy;
        igx = g->igx;
        igy = g->igy;
        pf_scale = g->pf_scale;
        pf_far = g->pf_far;
        x0 = g->x0;
        y0 = g->y0;
      } else if (role == 2) {
        speed_on = g->speed_on;
      }
    }
  }
  // the costmap the obstacle wave gathers from: the call's, or (LOG) the lane's own path's, loaded once
  const float* cm = a.cm;
  if constexpr (LOG) {
    if (a.cm_path && role == 3 && p < a.n) cm = a.cm_path[p];
  }

  std::conditional_t<LOG, StageLogT<WHEELS>, Stage<VEC>> r;
  stage_chunk<VEC, WHEELS, false, RAGGED>(a, r, sm, p0, 0, min(CT, Lld), tid);
  stage_chunk<VEC, WHEELS, true, RAGGED>(a, r, sm, p0, 0, min(CT, Lld), tid);
  __syncthreads();
  for (int t0 = 0; t0 < Lld; t0 += CT) {
    const int len = min(CT, Lld - t0);
    const int t1 = t0 + CT;
    const int len1 = min(CT, Lld - t1);  // <= 0: no next chunk
    if (len1 > 0) stage_chunk<VEC, WHEELS, false, RAGGED>(a, r, sm, p0, t1, len1, tid);

    const int te = min(t0 + len, L);  // this lane's waypoints of the chunk: [t0, te)
    if (role == 0) {
      const float* q = sm.a[0] + lane * ROW3;
      if (a.w_orient != 0.0f || a.orient) {  // (uniform) the path's last two waypoints, whichever chunks hold them
#pragma unroll
        for (int i = 0; i < 2; ++i) {
          const int tw = L - 2 + i;
          if (tw >= t0 && tw < te) {
            ex[i] = q[3 * (tw - t0)];
            ey[i] = q[3 * (tw - t0) + 1];
          }
        }
      }
      if (pf_far) {  // critics_warp.py:111-119: the terminal waypoint against the intermediate goal
        const int tl = L - 1;
        if (tl >= t0 && tl < te) acc = chain::path_far(q[3 * (tl - t0)], q[3 * (tl - t0) + 1], igx, igy, pf_scale);
      } else {  // :120-123
        const int tp = min(te, L - 1);
        for (int t = t0; t < tp; ++t) acc = acc + chain::path_near(q[3 * (t - t0)], q[3 * (t - t0) + 1], gx, gy);
      }
    } else if (role == 1) {
      const float* ql = sm.a[WHEELS ? 1 : 0] + lane * ROW3;
      const float* qr = sm.a[WHEELS ? 2 : 0] + lane * ROW3;
      for (int s = t0; s < te; s += 2) {  // t0 is even: s runs over the even waypoints
        const int k = 3 * (s - t0);
        const float cl[3] = {ql[k], ql[k + 1], ql[k + 2]};
        float cr[3] = {0.0f, 0.0f, 0.0f};
        if constexpr (WHEELS) {
          cr[0] = qr[k];
          cr[1] = qr[k + 1];
          cr[2] = qr[k + 2];
        }
        if (s >= 2 && s <= L - 2) {  // the term of t = s - 2 < L - 3
          float term = slope_one(pl, cl);
          if constexpr (WHEELS) {
            const float rs = slope_one(pr, cr);
            term = (term > rs) ? term : rs;
          }
          acc = acc + term;
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) {
          pl[i] = cl[i];
          pr[i] = cr[i];
        }
      }
    } else if (role == 2) {
      if (speed_on) {  // critics_warp.py:281-300
        const float* q = sm.v + lane * ROWV;
        for (int t = t0; t < te; ++t) acc = chain::speed(acc, a.vmax, q[t - t0]);
      }
    } else {
      const float* q = sm.a[0] + lane * ROW3;
      for (int t = t0; t < te; ++t) {  // critics_warp.py:244-262
        const float c = cm[chain::cm_index(a.hw, a.res_c, a.cm_size, q[3 * (t - t0)], q[3 * (t - t0) + 1])];
        const chain::ObstacleAcc oa = chain::obstacle(acc, col, c, a.thr, a.pen);
        acc = oa.acc;
        col = oa.col;
      }
    }
    __syncthreads();  // every wave is done with the staged chunk
    if (len1 > 0) {
      stage_chunk<VEC, WHEELS, true, RAGGED>(a, r, sm, p0, t1, len1, tid);
      __syncthreads();
    }
  }

  sm.term[role][lane] = acc;
  if (role == 3) sm.col[lane] = col;
  __syncthreads();
  if (role == 0 && p < a.n) {
    const float pf = sm.term[0][lane], sw = sm.term[1][lane], sp = sm.term[2][lane], ob = sm.term[3][lane];
    if (a.terms) *reinterpret_cast<float4*>(a.terms + 4 * (size_t)p) = make_float4(pf, sw, sp, ob);
    // critics_warp.py:44-82, as the rollout kernels' orientation_term; a path of one waypoint has no
    // last displacement: 0
    float po = 0.0f;
    if (L >= 2) po = chain::orientation(gx, gy, x0, y0, ex[0], ey[0], ex[1], ey[1]);
    if (a.orient) a.orient[p] = po;
    if (a.cost) {  // critics_warp.py:324-329
      float cost = chain::combine(a.w_path, a.w_slope, a.w_speed, a.w_obs, a.w_orient, pf, sw, sp, ob, po);
      if constexpr (LOG)
        if (L == 0) cost = 0.0f;  // an episode with no rows: cost 0 whatever the weights
      a.cost[p] = cost;
    }
    if (a.collisions) a.collisions[p] = sm.col[lane];
    if constexpr (LOG)
      if (a.rows_out) a.rows_out[p] = L;
  }
}

bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// One lane per path of a log: the whole-path form of mppi_path_metrics.h over the path's first L rows.
__global__ __launch_bounds__(64) void mppi_log_metrics_kernel(const float* __restrict__ log,
                                                               const int32_t* __restrict__ lengths, int len_step,
                                                               const int64_t* __restrict__ base_row, int stride,
                                                               int64_t n, PathMetrics* __restrict__ out) {
  const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (p >= n) return;
  const int L = min(max(lengths[(size_t)p * len_step], 0), stride);
  const size_t row0 = base_row ? (size_t)base_row[p] : (size_t)p * (size_t)stride;
  out[p] = path_metrics_rows(log + row0 * 8, 8, L);
}

// dm_atan2 (mppi_detmath.h) and the device library's atan2 on n pairs: the read-out behind
// mppi_detmath_atan2, which lets a test compare the device's bits with the numpy restatement's and
// measure the distance from the device's own arctangent.  One pair per lane, grid-stride.
__global__ __launch_bounds__(256) void mppi_atan2_probe_kernel(const double* __restrict__ y, const double* __restrict__ x,
                                                                int64_t n, double* __restrict__ dm,
                                                                double* __restrict__ dev) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
    dm[i] = dm_atan2(y[i], x[i]);
    dev[i] = atan2(y[i], x[i]);
  }
}

}  // namespace

hipError_t launch_atan2_probe(const double* y, const double* x, int64_t n, double* dm, double* dev, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!y || !x || !dm || !dev) return hipErrorInvalidValue;
  const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
  hipLaunchKernelGGL(mppi_atan2_probe_kernel, dim3(grid), dim3(256), 0, st, y, x, n, dm, dev);
  return hipGetLastError();
}

hipError_t launch_log_metrics(const float* log, const int32_t* lengths, int len_step, const int64_t* base_row,
                              int stride, int64_t n, PathMetrics* out, hipStream_t st) {
  if (n <= 0) return hipSuccess;
  if (!log || !lengths || !out || len_step < 1 || stride < 0) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mppi_log_metrics_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, st, log, lengths, len_step,
                     base_row, stride, n, out);
  return hipGetLastError();
}

hipError_t launch_score(const ScoreArgs& a, hipStream_t st) {
  if (a.n <= 0) return hipSuccess;
  if (a.log) {
    // stride 0: no run yet, every length is clamped to 0 and no row is read
    // (lw: the wheel log beside the log, rows of 24 bytes; rw stays null)
    if (!a.goals || !a.lengths || !a.cm || a.rw || a.stride < 0 || a.cm_size < 1 || a.len_step < 1 ||
        ((uintptr_t)a.log & 31) != 0 || ((uintptr_t)a.lw & 7) != 0 || (a.terms && !aligned16(a.terms)) ||
        (!a.base_row && a.n * (int64_t)std::max(a.stride, 1) >= ((int64_t)1 << 31)))
      return hipErrorInvalidValue;
    const dim3 grid((unsigned)((a.n + TP - 1) / TP));
    if (a.lw) {  // the slope wave on the wheel log's two contact paths
      if (a.base_row)
        hipLaunchKernelGGL((mppi_score_kernel<1, true, true, true>), grid, dim3(NT), 0, st, a);
      else
        hipLaunchKernelGGL((mppi_score_kernel<1, true, true>), grid, dim3(NT), 0, st, a);
    } else if (a.base_row) {
      hipLaunchKernelGGL((mppi_score_kernel<1, false, true, true>), grid, dim3(NT), 0, st, a);
    } else {
      hipLaunchKernelGGL((mppi_score_kernel<1, false, true>), grid, dim3(NT), 0, st, a);
    }
    return hipGetLastError();
  }
  if (!a.traj || !a.v || !a.cm || a.stride < 1 || a.cm_size < 1 || (a.lw == nullptr) != (a.rw == nullptr) ||
      (a.terms && !aligned16(a.terms)) || a.n * (int64_t)a.stride >= ((int64_t)1 << 31))
    return hipErrorInvalidValue;
  const unsigned blocks = (unsigned)((a.n + TP - 1) / TP);
  const bool wheels = a.lw != nullptr;
  // 16-byte loads when every row of every array starts 16-byte aligned
  const bool wide = a.stride % 4 == 0 && aligned16(a.traj) && aligned16(a.v) &&
                    (!wheels || (aligned16(a.lw) && aligned16(a.rw)));
  if (wide) {
    if (wheels)
      hipLaunchKernelGGL((mppi_score_kernel<4, true>), dim3(blocks), dim3(NT), 0, st, a);
    else
      hipLaunchKernelGGL((mppi_score_kernel<4, false>), dim3(blocks), dim3(NT), 0, st, a);
  } else {
    if (wheels)
      hipLaunchKernelGGL((mppi_score_kernel<1, true>), dim3(blocks), dim3(NT), 0, st, a);
    else
      hipLaunchKernelGGL((mppi_score_kernel<1, false>), dim3(blocks), dim3(NT), 0, st, a);
  }
  return hipGetLastError();
}

}  // namespace mppi
