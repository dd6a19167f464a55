// Host check of the bookkeeping of a batch's wheel log, wheel slope mode and path metrics
// (csrc/mppi_batch_wheels.h): which device tables exist when, for every combination of keep_log,
// wheel_log, scored, slope mode and metrics, for runs, task lists and tracking, and the refusals.  Built
// with ASan + UBSan by tests/test_batch_wheels_book.py; the header needs no HIP header.
#include <cstdio>

#include "mppi_batch_wheels.h"

using namespace mppi;

static int g_fail = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #cond);      \
      ++g_fail;                                                        \
    }                                                                  \
  } while (0)

static WheelTables tables(bool wlog, bool wacc, bool metrics) {
  WheelTables t;
  t.wlog = wlog;
  t.wacc = wacc;
  t.metrics = metrics;
  return t;
}

static BatchWheelBook book(bool wheel_log, bool slope_wheels, bool metrics) {
  BatchWheelBook b;
  CHECK(b.set_wheel_log(wheel_log, false, false) == kWheelOk);
  CHECK(b.set_score_options(slope_wheels ? kWheelSlopeWheels : kWheelSlopeBody, metrics, false, false) == kWheelOk);
  return b;
}

// a book that was never told anything: nothing exists, whatever runs
static void check_defaults() {
  BatchWheelBook b;
  CHECK(!b.wheel_log() && !b.slope_wheels() && !b.metrics() && !b.log_wheels());
  CHECK(!b.take_run().any() && !b.log_wheels());
  for (int scored = 0; scored < 2; ++scored)
    for (int keep = 0; keep < 2; ++keep) {
      CHECK(!b.take_list(scored, keep).any() && !b.list().any());
      CHECK(!b.take_tracking(keep).any() && !b.tracking().any());
    }
  CHECK(!b.can_score_wheels(false) && !b.can_score_wheels(true));
  // options turned on and off again before anything is set leave no trace
  CHECK(b.set_wheel_log(true, false, false) == kWheelOk && b.set_wheel_log(false, false, false) == kWheelOk);
  CHECK(b.set_score_options(kWheelSlopeWheels, true, false, false) == kWheelOk);
  CHECK(b.set_score_options(kWheelSlopeBody, false, false, false) == kWheelOk);
  CHECK(!b.take_run().any() && !b.take_list(true, true).any() && !b.take_tracking(true).any() && !b.log_wheels());
}

// every combination: 2^3 options x (run | list: scored x keep_log | tracking: keep_log)
static void check_every_combination() {
  for (int m = 0; m < 8; ++m) {
    const bool wl = m & 1, sw = m & 2, me = m & 4;
    {  // a run always logs: the wheel log follows the option alone; nothing online
      BatchWheelBook b = book(wl, sw, me);
      CHECK(b.take_run() == tables(wl, false, false));
      CHECK(b.log_wheels() == wl && b.can_score_wheels(true) == wl && b.can_score_wheels(false) == wl);
      CHECK(!b.list().any() && !b.tracking().any());
    }
    for (int scored = 0; scored < 2; ++scored)
      for (int keep = 0; keep < 2; ++keep) {
        BatchWheelBook b = book(wl, sw, me);
        // the wheel log needs the log; the chain and the metrics need a scored list, not a log
        const WheelTables want = tables(wl && keep, sw && scored, me && scored);
        CHECK(b.take_list(scored, keep) == want && b.list() == want);
        CHECK(!b.log_wheels());  // a list has its own arena: the run log's array is not its business
        CHECK(!b.tracking().any());
        b.clear_list();
        CHECK(!b.list().any() && b.wheel_log() == wl && b.slope_wheels() == sw && b.metrics() == me);
      }
    for (int keep = 0; keep < 2; ++keep) {
      BatchWheelBook b = book(wl, sw, me);
      const WheelTables want = tables(wl && keep, sw, me);
      CHECK(b.take_tracking(keep) == want && b.tracking() == want);
      CHECK(b.log_wheels() == (wl && keep));
      CHECK(!b.list().any());
      b.clear_tracking();
      CHECK(!b.tracking().any() && b.log_wheels() == (wl && keep));  // the kept log stays readable
    }
  }
}

// the log's parallel array belongs to whoever laid the log out last
static void check_log_ownership() {
  BatchWheelBook b = book(true, false, false);
  CHECK(b.take_run().wlog && b.log_wheels());
  // tracking without a log leaves the run's log and its array alone, and writes no wheel row
  CHECK(!b.take_tracking(false).wlog && b.log_wheels() && b.can_score_wheels(true));
  b.clear_tracking();
  // the option goes off: tracking that re-lays the log drops the array
  CHECK(b.set_wheel_log(false, false, false) == kWheelOk);
  CHECK(b.log_wheels());  // (until something lays the log out again)
  CHECK(!b.take_tracking(true).wlog && !b.log_wheels() && !b.can_score_wheels(true));
  b.clear_tracking();
  // on again: a log-free tracking takes no wheel log, a logged one does, and a later plain run keeps it
  CHECK(b.set_wheel_log(true, false, false) == kWheelOk);
  CHECK(!b.take_tracking(false).wlog && !b.log_wheels());
  b.clear_tracking();
  CHECK(b.take_tracking(true).wlog && b.log_wheels());
  b.clear_tracking();
  CHECK(b.take_run().wlog);
  CHECK(b.set_wheel_log(false, false, false) == kWheelOk);
  CHECK(!b.take_run().wlog && !b.log_wheels());
  // before any run the standing option answers for the (empty) paths
  BatchWheelBook c = book(true, false, false);
  CHECK(c.can_score_wheels(false) && !c.can_score_wheels(true));
  // a list set later does not change what an earlier list took
  BatchWheelBook d = book(true, true, true);
  CHECK(d.take_list(true, true) == tables(true, true, true));
  CHECK(d.set_score_options(kWheelSlopeBody, false, false, false) == kWheelOk);
  CHECK(d.list() == tables(true, true, true));
  CHECK(d.take_list(true, false) == tables(false, false, false));
}

static void check_refusals() {
  BatchWheelBook b = book(true, true, true);
  CHECK(b.set_wheel_log(false, true, false) == kWheelCampaign);
  CHECK(b.set_wheel_log(false, false, true) == kWheelTracking);
  CHECK(b.set_wheel_log(false, true, true) == kWheelCampaign);
  CHECK(b.set_score_options(kWheelSlopeBody, false, true, false) == kWheelCampaign);
  CHECK(b.set_score_options(kWheelSlopeBody, false, false, true) == kWheelTracking);
  CHECK(b.set_score_options(7, false, false, false) == kWheelSlopeMode);
  CHECK(b.set_score_options(-1, false, true, true) == kWheelSlopeMode);  // the argument first
  CHECK(b.wheel_log() && b.slope_wheels() && b.metrics());                // a refusal changes nothing
}

int main() {
  check_defaults();
  check_every_combination();
  check_log_ownership();
  check_refusals();
  if (g_fail) {
    std::printf("%d checks failed\n", g_fail);
    return 1;
  }
  std::printf("batch wheels book ok\n");
  return 0;
}
