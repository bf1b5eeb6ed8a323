// mpcekf_aging.hpp -- side-reaction losses per cell along the fused loop (mpcekf_aging_begin):
// the parameter and record rows, the kernel's arguments and the launches of mpcekf_aging.hip.
// Not a reference function: runMPC.m keeps phise_store above a margin; this integrates what a
// Tafel-type side reaction (lithium plating, SEI growth) draws at the overpotential and the
// temperature of every step.
#pragma once

#include <cstdint>

namespace mk {

constexpr int AG_MAXR = 4;  // reactions per context
constexpr int AG_NSRC = 2;  // sources: the EKF's estimate, the plant's truth
enum { AG_SRC_EST = 0, AG_SRC_PLANT };  // source index = bit of MPCEKF_AG_SRC_* (checked in mpcekf_host.cpp)
// rows of one reaction's parameter block [NAGP][n] and the ids of the record's fields, in the
// order of include/mpcekf.h's MPCEKF_AG_* / MPCEKF_AGR_* (checked in mpcekf_host.cpp)
enum { AG_I0 = 0, AG_U, AG_ALPHA, AG_EA, AG_GATE, NAGP };
enum { AGR_Q_SUM = 0, AGR_J_MAX, AGR_J_MAX_STEP, AGR_N_ON, AGR_STEPS, AGR_NSKIP, NAGR };
// The record is slot-major [AG_ROWS][n]: per source AG_MAXR blocks of the four per-reaction
// fields, then the source's STEPS and NSKIP.
constexpr int AG_PER_REACT = 4;
constexpr int AG_SRC_ROWS = AG_MAXR * AG_PER_REACT + 2;
constexpr int AG_ROWS = AG_NSRC * AG_SRC_ROWS;
// the record row of field f (AGR_*) of source s, reaction r
constexpr int ag_row(int s, int r, int f) {
  return s * AG_SRC_ROWS + (f < AG_PER_REACT ? r * AG_PER_REACT + f : AG_MAXR * AG_PER_REACT + (f - AG_PER_REACT));
}

struct KAging {
  const double *Tc;            // [n] s.Tc: the temperature the step used (degC)
  const double *phi[AG_NSRC];  // [n] this step's phise row (EST) / negPhise0 row (PLANT); null: source off
  const double *par;           // [nreact][NAGP][n]
  double *rec;                 // [AG_ROWS][n]
  double *rate;                // this step's [nsrc * nreact][n] block of the call's outputs, may be null
  int64_t n;
  int nreact;
  double F, R, Tref;           // the ROM's (KRom)
};

// the record of every cell reset (mpcekf_aging_begin)
int launch_aging_reset(double *rec, int64_t n, void *stream);
// one step's currents, after the kernel that wrote the step's phise row and before k_thermal
int launch_aging(const KAging &q, void *stream);

}  // namespace mk
