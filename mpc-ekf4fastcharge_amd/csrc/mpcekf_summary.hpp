// mpcekf_summary.hpp -- the per-cell charge summary along the fused loop (mpcekf_step_summary):
// the record's rows, the window of output rows the fused step writes into, and the launches
// of mpcekf_summary.hip.  Not a reference function: runMPC.m keeps whole trajectories
// (runMPC.m:55-69) and a script reduces them; this is that reduction, streamed on the device.
#pragma once

#include <cstdint>

namespace mk {

// Steps between two k_summary launches, and the rows of the ring the fused step's u / v /
// soc / phise / nexec (and one obs slot) outputs land in during mpcekf_step_summary: row k of
// a call is ring row k % SUM_WIN.  A constant of its own, independent of the flush period.
constexpr int SUM_WIN = 64;

// rows of the record [NSUM][n], in the order of include/mpcekf.h's MPCEKF_SUM_* (checked in
// mpcekf_host.cpp)
enum {
  SUM_SEEN = 0, SUM_STEPS, SUM_ERR_STEP, SUM_T_REACH, SUM_U_MIN, SUM_U_MIN_STEP, SUM_U_MAX, SUM_V_MAX,
  SUM_V_MAX_STEP, SUM_V_MIN, SUM_PHISE_MIN, SUM_PHISE_MIN_STEP, SUM_U_LAST, SUM_V_LAST, SUM_SOC_LAST,
  SUM_PHISE_LAST, SUM_U_SUM, SUM_NEXEC_SUM, SUM_NEXEC_MAX, SUM_NSAT, SUM_OBS_MIN, SUM_OBS_MIN_STEP, SUM_OBS_MAX,
  SUM_OBS_MAX_STEP, NSUM
};

struct KSum {
  double *rec;          // [NSUM][n] the record
  const double *reach;  // [n] SOC threshold of T_REACH (NaN: none)
  // the window: rows 0 .. nrows-1 of the ring, [SUM_WIN][n] each; obs may be null (no slot)
  const double *u, *v, *soc, *phise, *obs;
  const int *nexec;
  int64_t n;
  int nrows;     // 1 .. SUM_WIN
  int max_hild;  // NSAT counts nexec >= max_hild
};

// the record of every cell reset (mpcekf_summary_begin); no_reach: the thresholds set to NaN
int launch_summary_reset(double *rec, double *reach, bool no_reach, int64_t n, void *stream);
// the window's rows folded into the record; the step index continues from the record's SEEN
int launch_summary(const KSum &q, void *stream);

}  // namespace mk
