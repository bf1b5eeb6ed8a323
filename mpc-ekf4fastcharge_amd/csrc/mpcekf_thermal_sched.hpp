// mpcekf_thermal_sched.hpp -- the temperature schedule of the MPC limits (mpcekf_thermal_schedule):
// the schedule's device header, the kernels' arguments and the launches of
// mpcekf_thermal_sched.hip.  Not a reference function: runMPC.m:30-44 sets its limits once.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

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

#ifdef __HIPCC__
// The lookup, written once for every kernel that evaluates the schedule (k_sched,
// k_thermal_sched, k_thermal_couple_sched).  Every operation is one separately rounded fp64
// operation in the order include/mpcekf.h spells out: the including file sets
// `#pragma clang fp contract(off)` before its kernels.
#pragma clang fp contract(off)
// cell c's scheduled fields at temperature T
static __device__ __forceinline__ void sched_eval(const KSched &g, int64_t c, double T) {
  const SchedHdr *h = g.hdr;
  const int64_t n = g.n;
  const int nf = h->nf, ntab = h->ntab;
  const double T_lo = h->T_lo, T_hi = h->T_hi, Q = h->Q;
  const double x = (T - T_lo) / (T_hi - T_lo);
  double xc = x > 0.0 ? x : 0.0;  // NaN -> 0
  xc = xc < 1.0 ? xc : 1.0;
  const double s = xc * (double)(ntab - 1);
  int j = (int)s;
  if (j > ntab - 2) j = ntab - 2;
  const double f = s - (double)j;
  const double *tab = g.tab + (int64_t)g.set[c] * nf * ntab + j;
  for (int i = 0; i < SCHED_MAXF; ++i) {
    if (i >= nf) break;
    const double t0 = tab[(int64_t)i * ntab], t1 = tab[(int64_t)i * ntab + 1];
    const double val = t0 + f * (t1 - t0);
    g.lim[(int64_t)h->slot[i] * n + c] = h->crate[i] ? -Q * val : val;  // initMPC.m:66-67
    g.val[(int64_t)i * n + c] = val;
  }
}
#endif  // __HIPCC__

}  // namespace mk
