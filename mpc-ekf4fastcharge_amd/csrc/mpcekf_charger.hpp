// mpcekf_charger.hpp -- charger limits on pack strings along the fused loop
// (mpcekf_charger_begin): the record's and the parameters' rows, the kernel's arguments and the
// launches of mpcekf_charger.hip.  Not a reference function: runMPC.m charges one cell; a charger
// feeds a whole string and has a current and a power rating of its own.
#pragma once

#include <cstdint>

#include "mpcekf_balance.hpp"

namespace mk {

// rows of the parameters [NCHP][nstrings] and of the record [NCHR][nstrings], in the order of
// include/mpcekf.h's MPCEKF_CHP_* / MPCEKF_CH_* (checked in mpcekf_host.cpp)
enum { CHP_I_MAX = 0, CHP_P_MAX, NCHP };
enum { CH_STEPS = 0, CH_NCAP_I, CH_NCAP_P, CH_Q, CH_E, CH_CURTAIL, CH_P_MIN, CH_V_PEAK, CH_NVALID_MIN, NCHR };

struct KCharger {
  KPackBal b;         // k_pack_bal's arguments; b.par == nullptr: no balancer, only b.p (k_pack's) is read
  const double *vk;   // [n] s.vk: the plant voltage this step measured
  const double *par;  // [NCHP][n / series]
  double *rec;        // [NCHR][n / series]
  double *vstr;       // [n / series] this step's row of string voltages, may be null
  double *istr;       // [n / series] this step's row of string currents after the caps, may be null
  int *capby;         // [n / series] this step's row of -1 / 0 / 1 / 2, may be null
};

// the record to its start (counts and sums +0.0, P_MIN, V_PEAK and NVALID_MIN NaN)
int launch_charger_reset(double *rec, int64_t nstrings, void *stream);
// one step's string voltages, caps, balancing (with a balancer) and coupling, in launch_pack's or
// launch_pack_bal's place: after k_term, before the summary fold and k_thermal
int launch_charger(const KCharger &q, void *stream);

}  // namespace mk
