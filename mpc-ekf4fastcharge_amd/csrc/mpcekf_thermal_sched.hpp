// mpcekf_thermal_sched.hpp -- the temperature schedule of the MPC limits (mpcekf_thermal_schedule):
// the schedule's device header, the kernels' arguments and the launches of
// mpcekf_thermal_sched.hip.  Not a reference function: runMPC.m:30-44 sets its limits once.
#pragma once

#include <cstdint>

#include "mpcekf_thermal.hpp"

namespace mk {

enum { SCHED_MAXF = 6 };  // the schedulable fields: CRATE, U_MAX, DU_MIN, DU_MAX, V_MAX, PHISE_MIN

// The schedule as the kernels read it, in device memory: every quantity a replaced schedule may
// change lives here or in the buffers below, none in a kernel argument, so a captured graph
// replays the schedule in force.
struct SchedHdr {
  double T_lo, T_hi;      // the uniform grid's ends, degC
  double Q;               // rom.Q: the CRATE slot is u_min = -Q * val (fill_kcfg's expression)
  int nf, ntab, nsets, pad;
  int slot[SCHED_MAXF];   // field i's row LK_* of the limits record
  int crate[SCHED_MAXF];  // 1: field i is CRATE
};

struct KSched {
  const SchedHdr *hdr;
  const double *tab;  // [nsets][nf][ntab]
  const int *set;     // [n] each cell's table set, 0..nsets-1 (checked by the host)
  const double *Tc;   // [n] s.Tc
  double *lim;        // [NLIMK][n] mpcekf_set_limits' record: row slot[i] written
  double *val;        // [SCHED_MAXF][n] the values in force, mpcekf_config units: row i written
  int64_t n;
};

// the schedule at every cell's temperature as it stands (before a call's first step, and when a
// schedule is set)
int launch_sched(const KSched &g, void *stream);
// k_thermal's step of the model, then the schedule at the temperature it leaves: the last kernel
// of a step that another step of the same call follows
int launch_thermal_sched(const KTherm &q, const KSched &g, void *stream);

}  // namespace mk
