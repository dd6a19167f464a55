// C-ABI implementation (include/mppi.h): the multi-GPU group in one process.
#include <hip/hip_runtime.h>
#include <dlfcn.h>
#include <rccl/rccl.h>  // types only: RCCL is opened with dlopen by mppi_group_create
#include <sched.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "mppi.h"
#include "mppi_ctx.h"

using namespace mppi;
using namespace mppi::capi;

// ---- multi-GPU group in one process ----
// One context per member device over a contiguous, leaf-aligned shard of the global K (as
// mppi_amd/distributed.shard_bounds), Philox keyed by the global index; per step every member
// runs its partial step (rollout + its record), the records are all-gathered (RCCL, one
// ncclAllGather per member inside one group call, on the members' streams; members sharing a
// device exchange by device copies), and every member combines them in member order and runs the
// finish (identical controls everywhere; member 0's outputs are returned).

namespace {
struct RcclApi {
  void* h = nullptr;
  ncclResult_t (*comm_init_all)(ncclComm_t*, int, const int*) = nullptr;
  ncclResult_t (*comm_destroy)(ncclComm_t) = nullptr;
  ncclResult_t (*all_gather)(const void*, void*, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
  ncclResult_t (*group_start)() = nullptr;
  ncclResult_t (*group_end)() = nullptr;
  const char* (*error_string)(ncclResult_t) = nullptr;
  ncclResult_t (*comm_count)(const ncclComm_t, int*) = nullptr;
};
// RCCL from the process (torch may already hold one) or librccl.so.1; nullptr if unavailable
const RcclApi* rccl_api(std::string& why) {
  static RcclApi api;
  static bool tried = false;
  static std::string err;
  if (!tried) {
    tried = true;
    void* h = dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);
    if (!h) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
    if (!h) {
      err = std::string("RCCL not found: ") + dlerror();
    } else {
      api.h = h;
      api.comm_init_all = reinterpret_cast<decltype(api.comm_init_all)>(dlsym(h, "ncclCommInitAll"));
      api.comm_destroy = reinterpret_cast<decltype(api.comm_destroy)>(dlsym(h, "ncclCommDestroy"));
      api.all_gather = reinterpret_cast<decltype(api.all_gather)>(dlsym(h, "ncclAllGather"));
      api.group_start = reinterpret_cast<decltype(api.group_start)>(dlsym(h, "ncclGroupStart"));
      api.group_end = reinterpret_cast<decltype(api.group_end)>(dlsym(h, "ncclGroupEnd"));
      api.error_string = reinterpret_cast<decltype(api.error_string)>(dlsym(h, "ncclGetErrorString"));
      api.comm_count = reinterpret_cast<decltype(api.comm_count)>(dlsym(h, "ncclCommCount"));
      if (!api.comm_init_all || !api.comm_destroy || !api.all_gather || !api.group_start || !api.group_end)
        err = "RCCL lacks ncclCommInitAll / ncclAllGather / ncclGroupStart";
    }
  }
  why = err;
  return err.empty() ? &api : nullptr;
}
}  // namespace

struct mppi_group {
  int n = 0, E = 0;
  std::vector<mppi_ctx*> ctx;
  std::vector<int> dev;
  std::vector<int64_t> begin, count;
  std::vector<DeviceBuf<double>> rec;       // [E] this member's record (its device)
  std::vector<DeviceBuf<double>> gathered;  // [n * E] every member's record, member order (its device)
  std::vector<Event> ev;                    // copy exchange: this member's record is ready
  std::vector<double> empty_rec;  // the empty record (m = +inf, S = V = 0) for empty shards
  bool use_rccl = false;
  std::vector<ncclComm_t> comm;
  // Member threads (members 1..n-1; member 0 runs on the caller's thread).  Every member
  // enqueues its own partial step, exchange and finish and waits for its own completion word,
  // so the n enqueue paths (a few kernel launches + events each) run side by side instead of
  // one after another on the caller's thread (which skewed member n-1's rollout start by n
  // enqueue paths).  Handshake: the caller publishes the step (proj, step, out) and bumps `gen`;
  // each worker runs its member and decrements `pending`.  Workers spin for a short while after
  // each step (a control loop calls again within microseconds) and then sleep on the condition
  // variable.  One RCCL communicator per member, each driven only by its member's thread (the
  // one-thread-per-device use of ncclCommInitAll communicators: no group call needed).
  bool threaded = false;
  int spin_us = 0;      // how long a worker spins for the next step before it sleeps (granted_cpus)
  int cpus = 0;         // CPUs this process is granted
  bool selftest = false;  // mppi_group_selftest: host-only member steps (no GPU work at all), member
  int fail_member = -1;   // fail_member's failing
  std::vector<std::thread> workers;
  std::atomic<uint64_t> gen{0};
  std::atomic<int> pending{0};
  std::atomic<int> recorded{0};   // copy exchange: members whose record event is recorded
  std::atomic<int> sleepers{0};
  std::atomic<bool> stop{false};
  std::mutex mu;
  std::condition_variable cv;
  int cur_proj = 3;
  uint64_t cur_step = 0;
  mppi_outputs* cur_out = nullptr;
  std::vector<int> rc;
  std::vector<std::string> err;
};

namespace {

// Member i's partial step: rollout + its record (an empty member contributes the empty record).
int group_partial(mppi_group* g, int i, int proj, uint64_t step) {
  mppi_ctx* c = g->ctx[i];
  HIP_TRY(hipSetDevice(g->dev[i]));
  if (g->count[i] > 0) return mppi_step_partial(c, proj, step, g->rec[i]);
  HIP_TRY(hipMemcpyAsync(g->rec[i], g->empty_rec.data(), (size_t)g->E * sizeof(double), hipMemcpyHostToDevice,
                         c->stream));
  return MPPI_OK;
}

// Member i receives every member's record into gathered[i] (device copies, members that share
// a device or the device-copy mode): wait for each record's event, then a peer copy.
int group_copy_in(mppi_group* g, int i) {
  const size_t bytes = (size_t)g->E * sizeof(double);
  HIP_TRY(hipSetDevice(g->dev[i]));
  for (int j = 0; j < g->n; ++j) {
    HIP_TRY(hipStreamWaitEvent(g->ctx[i]->stream, g->ev[j], 0));
    HIP_TRY(hipMemcpyPeerAsync(g->gathered[i] + (size_t)j * g->E, g->dev[i], g->rec[j], g->dev[j], bytes,
                               g->ctx[i]->stream));
  }
  return MPPI_OK;
}

// Member i combines the n records in member order, runs the finish and waits for its outputs.
int group_finish(mppi_group* g, int i, mppi_outputs* out) {
  mppi_ctx* c = g->ctx[i];
  HIP_TRY(hipSetDevice(g->dev[i]));
  const Plan pl = c->last.have ? c->last.plan : make_plan(c);
  const int rc = enqueue_finish(c, pl, c->sb.st, g->gathered[i], g->n, 1, nullptr, true);
  if (rc) return rc;
  return copy_outputs(c, out);
}

// One member's whole step on its own thread (threaded groups).
int group_member_step(mppi_group* g, int i) {
  int rc = group_partial(g, i, g->cur_proj, g->cur_step);
  if (!g->use_rccl) {  // every member's record event must be recorded before anyone waits on it
    if (rc == MPPI_OK && hipEventRecord(g->ev[i], g->ctx[i]->stream) != hipSuccess)
      rc = fail(MPPI_EHIP, "group: hipEventRecord failed");
    g->recorded.fetch_add(1, std::memory_order_acq_rel);
    while (g->recorded.load(std::memory_order_acquire) < g->n) __builtin_ia32_pause();
    if (rc) return rc;
    rc = group_copy_in(g, i);
  } else {
    // every member enqueues its all-gather, also after a failed partial step (its record buffer
    // exists): the collective needs every rank, and a missing one would leave the other members'
    // gathers, finishes and completion waits pending (the step fails on this member's error)
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (!api) return fail(MPPI_EHIP, "group: " + why);
    const std::string saved = g_err;
    const ncclResult_t r = api->all_gather(g->rec[i], g->gathered[i], (size_t)g->E, ncclFloat64, g->comm[i],
                                           g->ctx[i]->stream);
    if (rc) {
      g_err = saved;
      return rc;
    }
    if (r != ncclSuccess)
      return fail(MPPI_EHIP, std::string("group: ncclAllGather: ") + (api->error_string ? api->error_string(r) : "error"));
  }
  if (rc) return rc;
  return group_finish(g, i, i == 0 ? g->cur_out : nullptr);
}

// mppi_group_selftest's member step: no GPU work, ~20 us of host time; member fail_member fails
int group_selftest_member(mppi_group* g, int i) {
  std::this_thread::sleep_for(std::chrono::microseconds(20));
  return i == g->fail_member ? fail(MPPI_EHIP, "injected failure") : MPPI_OK;
}

// CPUs this process may run on: its affinity set, bounded by its cgroup's CPU quota (cgroup v2)
int granted_cpus() {
  cpu_set_t set;
  int n = sched_getaffinity(0, sizeof(set), &set) == 0 ? CPU_COUNT(&set) : (int)std::thread::hardware_concurrency();
  if (FILE* f = std::fopen("/sys/fs/cgroup/cpu.max", "r")) {
    long q = 0, per = 0;
    if (std::fscanf(f, "%ld %ld", &q, &per) == 2 && q > 0 && per > 0) n = std::min<int>(n, std::max<long>(1, q / per));
    std::fclose(f);
  }
  return std::max(n, 1);
}

void group_worker(mppi_group* g, int i);

// Member threads: they spin (200 us, a control loop calls again within microseconds) only while the
// caller and every worker can hold a CPU of their own; on fewer granted CPUs they sleep at once.
void start_workers(mppi_group* g) {
  g->threaded = g->n > 1;
  g->rc.assign(g->n, MPPI_OK);
  g->err.assign(g->n, std::string());
  g->cpus = granted_cpus();
  g->spin_us = g->n < g->cpus ? 200 : 0;
  for (int i = 1; g->threaded && i < g->n; ++i) g->workers.emplace_back(group_worker, g, i);
}

void group_worker(mppi_group* g, int i) {
  if (!g->ctx.empty()) hipSetDevice(g->dev[i]);
  uint64_t seen = 0;  // the generation at start_workers (not a load here: a step posted before this
                      // thread ran would be taken as already seen, and the caller would wait for it)
  for (;;) {
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t now;
    for (int spin = 0; (now = g->gen.load(std::memory_order_acquire)) == seen && !g->stop.load(); ++spin) {
      if ((spin & 255) == 255 && std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(g->spin_us)) {
        std::unique_lock<std::mutex> lk(g->mu);
        g->sleepers.fetch_add(1);
        g->cv.wait(lk, [&] { return g->gen.load() != seen || g->stop.load(); });
        g->sleepers.fetch_sub(1);
      } else {
        __builtin_ia32_pause();
      }
    }
    if (g->stop.load()) return;
    seen = now;
    const int rc = g->selftest ? group_selftest_member(g, i) : group_member_step(g, i);
    g->rc[i] = rc;
    if (rc) g->err[i] = g_err;
    g->pending.fetch_sub(1, std::memory_order_acq_rel);
  }
}

// The caller's thread: publish the step, run member 0, wait for the others.
int group_step_threaded(mppi_group* g, int proj, uint64_t step, mppi_outputs* out) {
  g->cur_proj = proj;
  g->cur_step = step;
  g->cur_out = out;
  for (int i = 0; i < g->n; ++i) {
    g->rc[i] = MPPI_OK;
    g->err[i].clear();
  }
  g->recorded.store(0, std::memory_order_relaxed);
  g->pending.store(g->n - 1, std::memory_order_relaxed);
  {
    std::lock_guard<std::mutex> lk(g->mu);  // a worker about to sleep sees the new generation
    g->gen.fetch_add(1, std::memory_order_acq_rel);
  }
  if (g->sleepers.load() > 0) g->cv.notify_all();
  g->rc[0] = g->selftest ? group_selftest_member(g, 0) : group_member_step(g, 0);
  if (g->rc[0]) g->err[0] = g_err;
  while (g->pending.load(std::memory_order_acquire) > 0) __builtin_ia32_pause();
  for (int i = 0; i < g->n; ++i)
    if (g->rc[i]) return fail(g->rc[i], "group member " + std::to_string(i) + ": " + g->err[i]);
  return MPPI_OK;
}

}  // namespace

extern "C" {

int mppi_group_create(const mppi_params* params, int32_t n, const int32_t* devices, mppi_group** out) {
  if (!params || !devices || !out || n < 1) return fail(MPPI_EINVAL, "group: null argument or n < 1");
  *out = nullptr;
  const int64_t K = params->num_trajectories;
  if (K < 1) return fail(MPPI_EINVAL, "group: num_trajectories must be >= 1");
  auto* g = new mppi_group();
  g->n = n;
  g->E = 2 * params->num_iterations + 2;
  const int64_t leaves = (K + 255) / 256, per = (leaves + n - 1) / n;
  bool distinct = true;
  for (int i = 0; i < n; ++i) {
    const int64_t b = std::min<int64_t>(K, (int64_t)i * per * 256), e = std::min<int64_t>(K, (int64_t)(i + 1) * per * 256);
    g->begin.push_back(b);
    g->count.push_back(e - b);
    g->dev.push_back(devices[i]);
    for (int j = 0; j < i; ++j) distinct &= devices[j] != devices[i];
  }
  auto bail = [&](int rc) {
    mppi_group_destroy(g);
    return rc;
  };
  for (int i = 0; i < n; ++i) {
    mppi_params p = *params;
    p.num_trajectories = g->count[i] > 0 ? g->count[i] : 256;  // an empty shard's context serves the finish
    p.k_offset = params->k_offset + g->begin[i];
    mppi_ctx* c = nullptr;
    int rc = mppi_create(&p, devices[i], &c);
    if (rc) return bail(rc);
    g->ctx.push_back(c);
    DeviceBuf<double> r, ga;
    Event e;
    if (hipSetDevice(devices[i]) != hipSuccess || r.alloc((size_t)g->E * sizeof(double)) ||
        ga.alloc((size_t)n * g->E * sizeof(double)) || e.create(hipEventDisableTiming))
      return bail(fail(MPPI_EHIP, "group: device buffers"));
    g->rec.push_back(std::move(r));
    g->gathered.push_back(std::move(ga));
    g->ev.push_back(std::move(e));
  }
  g->empty_rec.assign((size_t)g->E, 0.0);
  g->empty_rec[0] = INFINITY;
  // MPPI_GROUP_RCCL: unset = RCCL between distinct devices (n > 1); 1 = also for one member
  // (exercises the RCCL exchange on a 1-GPU host); 0 = device copies only
  const char* env = std::getenv("MPPI_GROUP_RCCL");
  const int force = env ? std::atoi(env) : -1;
  if (distinct && ((n > 1 && force != 0) || force == 1)) {
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (!api) return bail(fail(MPPI_EHIP, "group: " + why));
    g->comm.assign(n, nullptr);
    const ncclResult_t r = api->comm_init_all(g->comm.data(), n, g->dev.data());
    if (r != ncclSuccess) {
      g->comm.clear();
      return bail(fail(MPPI_EHIP, std::string("group: ncclCommInitAll: ") +
                                      (api->error_string ? api->error_string(r) : "error")));
    }
    g->use_rccl = true;
  }
  try {  // member threads (n > 1): every member enqueues its own step
    start_workers(g);
  } catch (const std::exception& ex) {
    return bail(fail(MPPI_EHIP, std::string("group: worker threads: ") + ex.what()));
  }
  *out = g;
  return MPPI_OK;
}

int mppi_group_selftest(int32_t n, int32_t fail_member, int32_t steps, int64_t* info) {
  if (n < 2 || steps < 1 || !info) return fail(MPPI_EINVAL, "group selftest: n >= 2, steps >= 1, info");
  auto* g = new mppi_group();
  g->n = n;
  g->selftest = true;
  g->fail_member = fail_member;
  g->dev.assign(n, 0);
  try {  // (std::thread can throw: the exception must not cross the C ABI)
    start_workers(g);
  } catch (const std::exception& ex) {
    mppi_group_destroy(g);
    return fail(MPPI_EHIP, std::string("group selftest: worker threads: ") + ex.what());
  }
  int64_t done = 0, failed = 0, named = 0;
  for (int k = 0; k < steps; ++k) {
    const int rc = group_step_threaded(g, 3, (uint64_t)k, nullptr);
    ++done;
    failed += rc != MPPI_OK;
    named += rc != MPPI_OK && g_err.find("member " + std::to_string(fail_member) + ": injected") != std::string::npos;
  }
  const int64_t v[5] = {done, failed, named, (int64_t)g->workers.size(), g->spin_us};
  for (int i = 0; i < 5; ++i) info[i] = v[i];
  mppi_group_destroy(g);
  return MPPI_OK;
}

void mppi_group_destroy(mppi_group* g) {
  if (!g) return;
  if (!g->workers.empty()) {
    {
      std::lock_guard<std::mutex> lk(g->mu);
      g->stop.store(true);
    }
    g->cv.notify_all();
    for (auto& t : g->workers)
      if (t.joinable()) t.join();
  }
  std::string why;
  const RcclApi* api = g->comm.empty() ? nullptr : rccl_api(why);
  for (size_t i = 0; i < g->comm.size(); ++i)
    if (g->comm[i] && api) api->comm_destroy(g->comm[i]);
  for (mppi_ctx* c : g->ctx) mppi_destroy(c);  // (drains the member's streams: nothing reads the records after it)
  delete g;  // the members' records and events go with their handles
}

int mppi_group_size(mppi_group* g) { return g ? g->n : -1; }

int mppi_group_context(mppi_group* g, int32_t i, mppi_ctx** out) {
  if (!g || !out || i < 0 || i >= g->n) return fail(MPPI_EINVAL, "group: bad member index");
  *out = g->ctx[i];
  return MPPI_OK;
}

int mppi_group_shard(mppi_group* g, int32_t i, int64_t* begin, int64_t* count) {
  if (!g || i < 0 || i >= g->n) return fail(MPPI_EINVAL, "group: bad member index");
  if (begin) *begin = g->begin[i];
  if (count) *count = g->count[i];
  return MPPI_OK;
}

int mppi_group_info(mppi_group* g, int64_t* info, int32_t n) {
  if (!g || !info) return fail(MPPI_EINVAL, "null argument");
  int ranks = 0;
  if (g->use_rccl && !g->comm.empty()) {
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (api && api->comm_count) api->comm_count(g->comm[0], &ranks);
  }
  std::vector<int> devs(g->dev);
  std::sort(devs.begin(), devs.end());
  const int64_t distinct = std::unique(devs.begin(), devs.end()) - devs.begin();
  const int64_t v[7] = {g->n, distinct, g->use_rccl ? 1 : 0, ranks, g->threaded ? 1 : 0, g->spin_us, g->cpus};
  for (int i = 0; i < n && i < 7; ++i) info[i] = v[i];
  return MPPI_OK;
}

int mppi_group_step(mppi_group* g, int32_t proj, uint64_t step, mppi_outputs* out) {
  if (!g) return fail(MPPI_EINVAL, "null group");
  if (g->n == 1 && !g->use_rccl) return mppi_step(g->ctx[0], proj, step, out);
  if (proj != MPPI_PROJ_2D && proj != MPPI_PROJ_3D) return fail(MPPI_EINVAL, "proj must be 2 or 3");
  const int n = g->n;
  for (int i = 0; i < n; ++i) {
    const int rc = check_ready(g->ctx[i]);  // every member (an empty one runs the finish) needs its scene
    if (rc) return rc;
  }
  if (g->threaded) return group_step_threaded(g, proj, step, out);
  // one thread: every member's rollout and record, the exchange, every member's finish
  for (int i = 0; i < n; ++i) {
    const int rc = group_partial(g, i, proj, step);
    if (rc) return rc;
  }
  if (g->use_rccl) {
    std::string why;
    const RcclApi* api = rccl_api(why);
    if (!api) return fail(MPPI_EHIP, "group: " + why);
    ncclResult_t r = api->group_start();
    for (int i = 0; i < n && r == ncclSuccess; ++i)
      r = api->all_gather(g->rec[i], g->gathered[i], (size_t)g->E, ncclFloat64, g->comm[i], g->ctx[i]->stream);
    const ncclResult_t r2 = api->group_end();
    if (r != ncclSuccess || r2 != ncclSuccess)
      return fail(MPPI_EHIP, std::string("group: ncclAllGather: ") +
                                 (api->error_string ? api->error_string(r != ncclSuccess ? r : r2) : "error"));
  } else {
    for (int i = 0; i < n; ++i) {
      HIP_TRY(hipSetDevice(g->dev[i]));
      HIP_TRY(hipEventRecord(g->ev[i], g->ctx[i]->stream));
    }
    for (int i = 0; i < n; ++i) {
      const int rc = group_copy_in(g, i);
      if (rc) return rc;
    }
  }
  for (int i = 0; i < n; ++i) {
    mppi_ctx* c = g->ctx[i];
    HIP_TRY(hipSetDevice(g->dev[i]));
    const Plan pl = c->last.have ? c->last.plan : make_plan(c);
    const int rc = enqueue_finish(c, pl, c->sb.st, g->gathered[i], n, 1, nullptr, true);
    if (rc) return rc;
  }
  for (int i = 0; i < n; ++i) {
    HIP_TRY(hipSetDevice(g->dev[i]));
    const int rc = copy_outputs(g->ctx[i], i == 0 ? out : nullptr);
    if (rc) return rc;
  }
  return MPPI_OK;
}

}  // extern "C"
