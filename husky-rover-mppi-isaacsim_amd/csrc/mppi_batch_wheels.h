// The bookkeeping of a batch's wheel log, wheel slope mode and path metrics (mppi_batch_set_wheel_log /
// _set_score_options), as plain logic (no HIP header, so
// tests/native/batch_wheels_check.cpp checks it on the host): which options stand, what a run, a task
// list and tracking take of them when they are set, and therefore which device tables exist when.
// mppi_capi_batch.cpp allocates, frees and launches by these answers alone.
//
// The rules.  The options are read when a run starts, a list is set or tracking is set, and stay what
// that run, list or tracking took until it is replaced or cleared.
//   wheel log   beside a log only: a run always logs; a list or tracking only with keep_log.
//   wheel chain, metrics   online, for what is scored as it runs: a scored list, or tracking; a plain
//               list takes neither.  Neither needs a log.
//   The log `log` (mppi_batch_run's, and tracking's with keep_log) has one parallel array: it holds the
//   contacts of the rows of whoever laid the log out last, or does not exist.  Tracking without keep_log
//   leaves the log, and so the array, as they are.
//   Both setters are refused while a campaign is unfinished or tracking is set.
#pragma once

namespace mppi {

enum WheelError { kWheelOk = 0, kWheelCampaign, kWheelTracking, kWheelSlopeMode };
constexpr int kWheelSlopeWheels = 0, kWheelSlopeBody = 1;  // mppi_slope_mode (include/mppi.h)

// The tables one run, list or tracking owns: each exists iff its flag is set.
struct WheelTables {
  bool wlog = false;     // the contacts beside the log rows
  bool wacc = false;     // [E] the previous even contacts: the online slope chain in its wheel form
  bool metrics = false;  // [E] the online metrics state, and the result rows beside the score rows
  bool any() const { return wlog || wacc || metrics; }
  bool operator==(const WheelTables& o) const { return wlog == o.wlog && wacc == o.wacc && metrics == o.metrics; }
};

class BatchWheelBook {
 public:
  // ---- the options as last set
  WheelError set_wheel_log(bool on, bool campaign_unfinished, bool tracking) {
    if (campaign_unfinished) return kWheelCampaign;
    if (tracking) return kWheelTracking;
    wheel_log_ = on;
    return kWheelOk;
  }
  WheelError set_score_options(int slope_mode, bool metrics, bool campaign_unfinished, bool tracking) {
    if (slope_mode != kWheelSlopeWheels && slope_mode != kWheelSlopeBody) return kWheelSlopeMode;
    if (campaign_unfinished) return kWheelCampaign;
    if (tracking) return kWheelTracking;
    slope_wheels_ = slope_mode == kWheelSlopeWheels;
    metrics_ = metrics;
    return kWheelOk;
  }
  bool wheel_log() const { return wheel_log_; }
  bool slope_wheels() const { return slope_wheels_; }
  bool metrics() const { return metrics_; }

  // ---- what each way of running takes
  // mppi_batch_run lays the log out anew: the parallel array exists from here on iff the option is on.
  WheelTables take_run() {
    log_wheels_ = wheel_log_;
    WheelTables t;
    t.wlog = log_wheels_;
    return t;
  }
  // mppi_batch_set_tasks / _set_tasks_scored (a plain list always keeps its log)
  WheelTables take_list(bool scored, bool keep_log) {
    list_ = WheelTables{};
    list_.wlog = keep_log && wheel_log_;
    list_.wacc = scored && slope_wheels_;
    list_.metrics = scored && metrics_;
    return list_;
  }
  void clear_list() { list_ = WheelTables{}; }
  // mppi_batch_set_tracking; with keep_log it lays the log out anew, as a run does
  WheelTables take_tracking(bool keep_log) {
    if (keep_log) log_wheels_ = wheel_log_;
    trk_ = WheelTables{};
    trk_.wlog = keep_log && log_wheels_;
    trk_.wacc = slope_wheels_;
    trk_.metrics = metrics_;
    return trk_;
  }
  void clear_tracking() {  // (the log and its parallel array stay readable)
    trk_ = WheelTables{};
  }

  // ---- what stands
  bool log_wheels() const { return log_wheels_; }   // the log's parallel array exists
  const WheelTables& list() const { return list_; }
  const WheelTables& tracking() const { return trk_; }
  // MPPI_SLOPE_WHEELS after the run (mppi_batch_score_ex): the log's rows have contacts; before any run
  // (no log yet: every path has no rows) the standing option decides
  bool can_score_wheels(bool has_log) const { return has_log ? log_wheels_ : wheel_log_; }

 private:
  bool wheel_log_ = false, slope_wheels_ = false, metrics_ = false;
  bool log_wheels_ = false;
  WheelTables list_, trk_;
};

}  // namespace mppi
