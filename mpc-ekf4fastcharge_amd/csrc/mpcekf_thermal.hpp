// mpcekf_thermal.hpp -- the per-cell lumped thermal model of the fused loop
// (mpcekf_thermal_begin): the record's rows, the kernel's arguments and the launches of
// mpcekf_thermal.hip.  Not a reference function: runMPC.m:85-92 passes a temperature TC it is
// given; this model makes TC a state that follows from the current and the voltage of each step.
#pragma once

#include <cstdint>

namespace mk {

// rows of the parameter block [NTH][n] and of the record [NTHR][n], in the order of
// include/mpcekf.h's MPCEKF_TH_* / MPCEKF_THR_* (checked in mpcekf_host.cpp).  Row THR_T of
// the record is never stored: T is s.Tc itself.
enum { TH_CTH = 0, TH_RTH, TH_TAMB, NTH };
enum { THR_T = 0, THR_T_MAX, THR_T_MAX_STEP, THR_T_MIN, THR_HEAT_SUM, THR_STEPS, THR_NHELD, NTHR };

struct KTherm {
  double *Tc;            // [n] s.Tc: read, advanced (or held) in place
  const double *vk;      // [n] s.vk: the plant's Vcell of this step
  const double *SOCn;    // [n] cellState.SOCnAvg after the step
  const int *status;     // [n] MPCEKF_ST_*: a cell in error has NaN outputs, so its v is NaN here
  const double *uk;      // [n] s.uk after the step: the current the next step applies
  double *iapp;          // [n] the current this step applied; rewritten with uk for the next step
  const double *par;     // [NTH][n]
  const double *ocv;     // [nocv] open-circuit voltage over cell SOC 0..1, uniform grid
  double *rec;           // [NTHR][n]
  double *temp, *heat;   // [n] this step's rows of the call's outputs, may be null
  int64_t n;
  int nocv;
  double th0n, th100n, Ts;
};

// the record of every cell reset (mpcekf_thermal_begin)
int launch_thermal_reset(double *rec, int64_t n, void *stream);
// one step of the model, after the fused step's last kernel
int launch_thermal(const KTherm &q, void *stream);

}  // namespace mk
