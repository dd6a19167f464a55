// Private header of the C-ABI implementation (mppi_capi*.cpp): the context as owned parts, and the
// few internal functions that more than one of those files calls (namespace mppi::capi).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstring>
#include <functional>
#include <memory>
#include <string>
#include <unordered_map>

#include "mppi.h"
#include "mppi_costmap.h"
#include "mppi_handles.h"
#include "mppi_kernels.h"
#include "mppi_score.h"
#include "mppi_slots.h"

// The internal names stay out of the library's exported symbols (include/mppi.h is the whole
// exported set), and calls between the host files are direct.
#define MPPI_INTERNAL __attribute__((visibility("hidden")))

namespace mppi {
namespace capi MPPI_INTERNAL {

extern thread_local std::string g_err;  // mppi_last_error

int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                      \
  do {                                                                                     \
    hipError_t e_ = (hipError_t)(expr);                                                    \
    if (e_ != hipSuccess)                                                                  \
      return fail(MPPI_EHIP, std::string(#expr) + " failed: " + hipGetErrorString(e_));    \
  } while (0)

constexpr size_t kLdsBytes = 160 * 1024;
// (mppi::kTailSlots deferred optimal rollouts in flight: the tail of step i may run until step
// i + kTailSlots is issued; beside the next rollouts it gets only the issue slots their waves leave)

struct Plan {
  int traj_per_block = 256;
  int block = 256, blocks = 0;
  int grid = 0;  // rollout workgroups (the role-split kernel runs blocks beyond one per CU in turn)
  int W = 1, Wr = 1;  // the DEM window every lane of the step can touch (mppi_get_launch_info)
  size_t lds_bytes = 0, fin_lds_bytes = 0, fin_tree_bytes = 0;
  int ucache_steps = 0;   // pair kernel: steps whose sampled controls stay in LDS for the leaf
  bool roles = false;     // the role-split rollout kernel (mppi_rollout_roles_kernel)
};

// DEM with its normals table.  Z is owned (mppi_set_dem) or borrowed (mppi_set_dem_device).
struct Dem {
  DeviceBuf<float> Z;
  DeviceBuf<float4> ntab;  // per-cell normals of the DEM, (rows+1) x (cols+1) (mppi_normal_table_kernel)
  int rows = 0, cols = 0;
  float x_min = 0, y_min = 0, res = 0;
  float rinv_res = 0;  // verified division-by-constant reciprocal of res (0 = use the IEEE division)
};

// Owner of the costmap build's scratch; view() is the kernels' argument block (mppi_costmap.h).
struct CostmapBuffers {
  DeviceBuf<uint8_t> occ;
  DeviceBuf<int32_t> first, last, g2, d2, range;
  DeviceBuf<uint32_t> lines;
  DeviceBuf<double> obs, xs;
  DeviceBuf<int32_t> hz_tab;  // hazard build: ci[cols] then rj[rows] (mppi_hazard.h)
  DeviceBuf<uint8_t> mask;    // hazard build: [size*size] H0 / H1 / disc bits, when the caller asks for them
  size_t cells_cap = 0;
  // Let go of the per-cell planes before larger ones are allocated (`lines` alone is 64 bytes per cell).
  void drop_planes() {
    for (DeviceBuf<int32_t>* b : {&first, &last, &g2, &d2}) b->reset();
    occ.reset();
    lines.reset();
    cells_cap = 0;
  }
  CostmapScratch view() const {
    CostmapScratch sc;
    sc.occ = occ;
    sc.first = first;
    sc.last = last;
    sc.g2 = g2;
    sc.d2 = d2;
    sc.range = range;
    sc.lines = lines;
    sc.obs = obs;
    sc.xs = xs;
    sc.cells_cap = cells_cap;
    sc.obs_cap = obs.cap();
    sc.xs_cap = xs.cap();
    return sc;
  }
};

struct Costmap {
  DeviceBuf<float> cm;
  int size = 0;
  float hw = 0, res = 0;
  float rinv_res = 0;      // verified reciprocal of res (0 = use the IEEE division)
  CostmapBuffers scratch;  // mppi_build_costmap scratch
};

// State, nominal sequence and the buffers one step reads and writes.
struct StepBuffers {
  mppi_state st{};
  bool have_state = false;
  // nominal sequence double buffer: u_nom[cur] is read by the next step
  DeviceBuf<float> u_nom[2];
  int cur = 0;
  DeviceBuf<float> cost;
  DeviceBuf<double> nodes;
  DeviceBuf<float> rec_m;  // [nodes_cap / E] the records' m, contiguous
  size_t nodes_cap = 0;    // doubles of `nodes`; rec_m, scratch0 and scratch1 are sized with it (ensure_nodes)
  DeviceBuf<double> scratch0, scratch1;
  DeviceBuf<float> ustore;    // sampled controls of the current step [blocks][2][H][block]
  PinnedBuf<float> stage;     // pinned [16H]: the finish kernel stores the outputs here directly
  PinnedBuf<unsigned> done;   // pinned completion word (FinishArgs::done)
  unsigned seq = 0;
  unsigned wait_seq = 0;  // the completion word wait_done waits for
  std::unique_ptr<float[]> out_host;  // [16H] last complete outputs (host memory)
  DeviceBuf<float> inj1, inj2;
  // finish: column-split u_opt slice records / first tree level, arrival counter
  DeviceBuf<double> level1;          // finish kernel first-level records
  DeviceBuf<unsigned> level1_cnt;    // [0]: finish handoff, [16]: the server's record count
  DeviceBuf<unsigned long long> uopt;  // [2H] the column-split finish's tagged u_opt words
  DeviceBuf<uint64_t> clk;  // [4] chain clock stamps of the last sampled rollout (RolloutArgs::clk)
};

// The sampling normals' slots: buffers, fill events and the stream the speculative fills run on.
// Which slot holds which step is `pol`'s (mppi_slots.h); no other code loops over the slots.
struct NormalsSlots {
  EpsPolicy pol;
  DeviceBuf<float> buf[kEpsSlots];
  size_t cap = 0;  // floats per slot
  Event ev[kEpsSlots];
  Stream stream;       // the noise stream (least priority)
  Event ev_prev_roll;  // recorded after the last rollout that read a slot
  // where the next steps' normals are ordered on the context stream (separate launches, partial
  // steps): after the rollout (an event marker between the rollout and the finish, ~5 us on the
  // step's path) or after the finish (the noise then runs into the next rollout of a back-to-back
  // caller).  after: -1 by the call's cadence (default: after the finish for a call more than
  // half the idle limit after the last one returned, a simulator frame), 0 / 1 forced (mppi_set_option "eps_after")
  int after = -1;
  bool late = false;  // this step's choice

  // Size every slot for `need` floats; `main` and the noise stream are drained before a slot is freed.
  int ensure(size_t need, hipStream_t main);
  // Every fill in flight must finish before a slot is reused for a step no slot holds: wait on the
  // host (sync) or order `st` after it.
  int settle_all(hipStream_t st, bool sync);
  // Slot `slot`'s fill (if pending) before a rollout on `st` reads it.
  int settle(int slot, hipStream_t st, bool sync);
};

// Deferred optimal rollouts (mppi_set_async_tail): side stream, per-slot buffers and events.
// Which slot is next, claimed or done is `pol`'s (mppi_slots.h).
struct TailRing {
  TailRingPolicy<kTailSlots> pol;
  bool async = false;
  Stream stream;
  Event ev_fin_done;
  Event ev[kTailSlots];               // per slot: tail done
  hipStream_t ts[kTailSlots] = {};    // the stream that slot's tail was launched on (not owned)
  DeviceBuf<float> in[kTailSlots];    // device [3H] per slot
  PinnedBuf<float> host[kTailSlots];  // pinned [12H] per slot (written by the kernel)
  // the server's tail of the last step, launched once its completion word was seen (at the next
  // step's command, or when its outputs are wanted): no kernel waits on the GPU for its inputs
  FinishArgs def{};

  // Wait until no tail of any slot can still run (sync_tail).
  int drain();
};

// Resident step server (mppi_step_server_kernel): sampled steps of the role-split plan run on one
// resident launch that polls the command block `cmd` (pinned) instead of one launch per step
// (mppi_set_option "resident", env MPPI_RESIDENT).  It exits after idle_us without a command, on
// the command's stop slot == its launch id (every other call on the context stops it first: quiesce) or on a
// failed step.  resident 1 (default): only back-to-back calls (within half the idle limit of the
// last step's return) keep or start it, a step after a longer gap runs as separate launches (the
// caller's frame cadence: a launch of the server per frame costs more than the launches it saves);
// 2: every step whose plan fits; 0: never.
struct Server {
  int resident = 1;
  PinnedBuf<ServerCmdWire> cmd;          // pinned: the command's tagged slots (mppi_cmd.h)
  DeviceBuf<unsigned long long> relay;  // device [kCmdSlots]: the head's relay of them (ServerArgs::relay)
  // (two flags, not one state: both are true while a new launch is queued behind a leaving one)
  bool running = false;
  bool exiting = false;    // a stop was posted and the launch may not have retired yet
  unsigned launch_id = 0;  // the running (or last) launch's id: its stop word
  double last_return_us = 0;  // host time the last step returned (0: none yet)
  int b2b_calls = 0;          // consecutive back-to-back steps (resident 1)
  int64_t fallbacks = 0;      // server steps whose finish gave up, rerun as separate launches
  int64_t cadence_steps = 0;  // steps the server's plan fits that ran as separate launches (resident 1)
  int proj = 0;
  double last_us = 0;      // host time the server last became idle (its last step completed, or launch)
  uint64_t idle_us = 200;  // (bench.py cadence leg: at 2000 a simulator kernel needing LDS waited
                           // out the idle server every frame)
  int64_t launches = 0, steps = 0, failed = 0;
  int64_t relaunches = 0;  // commands a leaving server did not take, served by a relaunch (wait_done)
  int cmd_noise = -1;      // the normals slot the last command asked the server's noise phase for
  int fail_kind = 0;       // the last failed wait: 1 finish gave up, 2 launch retired, 3 timeout
  bool warned = false;
  // the server launch of the command wait_done waits for (a relaunch serves the same command)
  bool cmd_live = false;
  Plan pl;
  int P = 0, ncol = 0, groups = 0;
  size_t lds = 0;
  unsigned exit_after = 0;  // test hook mppi_set_option("server_exit_after"): the next launch's head
                            // leaves after serving this many commands (0: off)
  // a finish's record wait bound (100 MHz ticks; mppi_set_option): 1 ms, many step periods.  Every
  // workgroup of a running server is resident, so its records arrive within the rollouts' end spread
  // (~4 us at C3); a fresh launch whose workgroups cannot all get CUs (another stream's kernels hold
  // some) would wait for them, while the workgroups it has hold theirs: past the bound the step is
  // rerun as separate launches, which need no co-residency (step_impl)
  uint64_t fin_wait_ticks = 100000ull;
};

// Kernel timing (mppi_set_timing) and the host-side step timeline.
struct Timing {
  int mode = 0;  // 1: rollout, finish and tail events; 2: rollout only, no host wait (mppi_set_timing)
  Event ev[6];
  Event ev_side[2];  // timing mode 2: the side streams' work so far
  bool roll_pending = false, fin_pending = false, tail_pending = false;
  double t_roll = 0, t_fin = 0, t_tail = 0;
  int64_t launches = 0, tail_launches = 0;
  double score_ms = 0;  // HIP-event time of the last scoring kernel (mppi_get_score_ms)
  // host-side step timeline (env MPPI_HOST_TRACE=1, printed by mppi_destroy): per step the host
  // times (us) of 6 marks (trace_mark), summed as phases over the steps and kept for the last 8
  bool trace = false;
  double tr_m[6] = {}, tr_sum[6] = {}, tr_log[8][6] = {}, tr_prev = 0;
  long tr_n = 0;
};

// tiled bilinear binning scratch
struct BinScratch {
  DeviceBuf<int> tile_of;  // per-chunk tile histograms [chunks][tiles]
  DeviceBuf<int> counts;   // counts [nt], then the tile-row cursors of the two-level scatter [nt]
  DeviceBuf<int> cursor;
  // two-level binning: the tile-row-sorted queries [n] and the tile-row cursors [rows of tiles]
  DeviceBuf<float> cx, cy;
  DeviceBuf<int32_t> ci;
};

// What the last step ran (mppi_get_launch_info) and what a dump re-runs.
struct LastStep {
  // the finish the last step ran: 1 column-split, 0 record tree
  int fin_kind = -1, fin_P = 0, fin_ncol = 0, fin_groups = 0;
  bool resident = false;  // the last step ran on the resident server (mppi_get_launch_info info[11])
  bool have = false;
  int proj = 3, mode = 0;
  uint64_t step = 0;
  mppi_state state{};
  int nominal = 0;
  Plan plan;
};

}  // namespace capi
}  // namespace mppi

struct mppi_ctx {
  mppi_params p{};
  mppi_critics crit{MPPI_SLOPE_WHEELS, 0.0f};  // the critic set (mppi_set_critics)
  mppi_sampling samp{0, 0, 0.0f};              // the sampling plan (mppi_set_sampling)
  int device = 0;
  mppi::Stream stream;  // owned, or the caller's (mppi_set_stream)
  int prio_least = 0, prio_greatest = 0;
  int num_cus = 256;  // compute units of the device (hipDeviceAttributeMultiprocessorCount)
  // finish: 1 = column-split kernel (mppi_colfin_kernel) where it applies, 0 = the record tree
  // (mppi_set_option "record_tree_finish")
  int colfin = 1;
  int roles = -1;     // rollout kernel: -1 auto (role split at <= 1 workgroup per CU), 0 pair, 1 roles (MPPI_ROLES)
  mppi::DeviceBuf<unsigned> cdiv_bad;  // device counter for launch_cdiv_verify
  std::unordered_map<uint32_t, float> cdiv_cache;  // divisor bits -> verified y (0: none)
  // test hook mppi_set_option("verified_reciprocal"): false makes verified_reciprocal hand out 0,
  // so every cell index of the DEM and the costmap takes the IEEE division
  bool use_cdiv = true;
  mppi::capi::Dem dem;
  mppi::capi::Costmap cmap;
  mppi::capi::StepBuffers sb;
  mppi::capi::NormalsSlots ns;
  mppi::capi::TailRing tail;
  mppi::capi::Server srv;
  mppi::capi::Timing tm;
  mppi::capi::BinScratch bin;
  mppi::capi::LastStep last;
};

namespace mppi {
namespace capi MPPI_INTERNAL {

inline int H_of(const mppi_ctx* c) { return c->p.num_iterations; }
inline int E_of(const mppi_ctx* c) { return 2 * c->p.num_iterations + 2; }
inline size_t up16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// (Re)allocate device buffer b for `bytes` when its capacity is short.  The old contents are
// dropped; `st`, which may still read the old buffer, is synchronised first.
template <class T>
int grow(DeviceBuf<T>& b, size_t bytes, hipStream_t st) {
  if (bytes <= b.cap()) return MPPI_OK;
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(b.alloc(bytes));
  return MPPI_OK;
}

// mppi_capi.cpp
int check_ready(mppi_ctx* c);
Plan make_plan(const mppi_ctx* c);
int quiesce(mppi_ctx* c);
// empty when the set is valid for a context of H steps, else the message naming the field
std::string critics_error(const mppi_critics& k, int H);
// the same for a sampling plan on a context whose trajectory 0 is global k_offset
std::string sampling_error(const mppi_sampling& s, int64_t k_offset);
// the plan as the generator takes it (g formed here, once)
SamplePlan device_plan(const mppi_sampling& s);
int verified_reciprocal(mppi_ctx* c, float b, float* y_out);
void state_fields(const mppi_params& p, const mppi_state& st, ServerCmd& d);
void fill_rollout(const mppi_ctx* c, const Plan& pl, const mppi_state& st, uint64_t step, const float* unom,
                  RolloutArgs& a);
void fill_finish(const mppi_ctx* c, const Plan& pl, const mppi_state& st, FinishArgs& f);
int enqueue_rollout(mppi_ctx* c, int proj, uint64_t step, int mode, const Plan& pl, const float* unom,
                    const mppi_state& st, const RolloutArgs* dump_args, int* spec_slot = nullptr);
int enqueue_finish(mppi_ctx* c, const Plan& pl, const mppi_state& st, const double* recs, int n, int mode,
                   double* record_out, bool timed);
int copy_outputs(mppi_ctx* c, mppi_outputs* out);
int install_dem(mppi_ctx* c, int32_t rows, int32_t cols, float x_min, float y_min, float resolution,
                const std::function<int(float*)>& fill);
// mppi_capi_batch.cpp
mppi_ctx* batch_context(mppi_batch* b);
int batch_dem_slot(const mppi_batch* b, int32_t slot);  // MPPI_EINVAL, naming the slot, outside the table
int batch_fill_dem(mppi_batch* b, int32_t slot, const char* who, const std::function<int(float*)>& fill);
// mppi_capi_dem.cpp: n craters into `dst` (device, grid x grid floats) on `st`, copied to out_host when
// given; ends synchronised.  The factor tables live for the call only (2 x 2n x grid doubles).
int build_dem_into(hipStream_t st, const double* craters, int32_t n, int32_t grid, double half_width,
                   const float* base_host, float* dst, float* out_host, int32_t variant);
// mppi_capi_costmap.cpp
// heights on the device with their geometry, as a hazard build reads them (a context's DEM or a batch's slot)
struct DemView {
  const float* Z = nullptr;
  int32_t rows = 0, cols = 0;
  float x_min = 0, y_min = 0, res = 0;
};
inline DemView dem_view(const Dem& d) { return DemView{d.Z.get(), d.rows, d.cols, d.x_min, d.y_min, d.res}; }
// hz == nullptr: the rock-only build (dem and mask_host are not looked at)
int build_costmap_into(mppi_ctx* c, const double* obstacles, int32_t n, int32_t size, double half_width,
                       double origin_x, double origin_y, double r_robot, int32_t power, int32_t metric, float* dst,
                       float* out_host, const mppi_hazard* hz = nullptr, const DemView* dem = nullptr,
                       uint8_t* mask_host = nullptr);
// mppi_capi_score.cpp
int run_score(mppi_ctx* c, const ScoreArgs& a);

}  // namespace capi
}  // namespace mppi
