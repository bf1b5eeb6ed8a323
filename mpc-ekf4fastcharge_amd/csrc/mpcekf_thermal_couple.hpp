// mpcekf_thermal_couple.hpp -- heat conduction between neighbouring cells of a pack string
// (mpcekf_thermal_couple): the record's rows, the kernels' arguments and the launches of
// mpcekf_thermal_couple.hip.  Not a reference function: the thermal model of
// mpcekf_thermal.hip exchanges heat with each cell's own ambient only.
#pragma once

#include <cstdint>

#include "mpcekf_thermal.hpp"
#include "mpcekf_thermal_sched.hpp"

namespace mk {

// rows of the record [NTCR][n], in the order of include/mpcekf.h's MPCEKF_TCR_* (checked in
// mpcekf_host.cpp)
enum { TCR_NB_SUM = 0, TCR_DT_MAX, TCR_DT_MAX_STEP, NTCR };

struct KCouple {
  const double *rlink;    // [n] K/W between cell c and c + 1; +inf: no link; a string's last entry is never read
  double *rec;            // [NTCR][n]
  const double *snap_in;  // [n] every cell's temperature as this step found it: the neighbours are read here
  double *snap_out;       // [n] the temperature this step leaves, advanced or held: the next step's snap_in
  double *cond;           // [n] this step's row of the call's output, may be null
  int series;             // cells per string
};

// the record of every cell reset (mpcekf_thermal_couple, and a second mpcekf_thermal_begin)
int launch_couple_reset(double *rec, int64_t n, void *stream);
// a fused call's seed: s.Tc as the call finds it into the snapshot its first step reads
int launch_couple_seed(const double *Tc, double *snap, int64_t n, void *stream);
// one step of the model with conduction, in k_thermal's place
int launch_thermal_couple(const KTherm &q, const KCouple &h, void *stream);
// the same, then the schedule at the temperature it leaves, in k_thermal_sched's place
int launch_thermal_couple_sched(const KTherm &q, const KCouple &h, const KSched &g, void *stream);

}  // namespace mk
