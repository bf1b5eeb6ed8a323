// mpcekf_term.hpp -- charge termination along the fused loop (mpcekf_term_begin): the record's
// rows, the kernels' arguments and the launches of mpcekf_term.hip.  Not a reference function:
// runMPC.m steps its one cell for a fixed 3,000 s; a charger stops at a SOC, on a tapered current
// or on a temperature, and a string stops with its first cell.
#pragma once

#include <cstdint>

namespace mk {

// rows of the record [NTMR][n], in the order of include/mpcekf.h's MPCEKF_TM_* (checked in
// mpcekf_host.cpp)
enum { TM_STATE = 0, TM_DONE_STEP, TM_REASON, TM_SOC_DONE, TM_U_DONE, TM_T_DONE, TM_REST, TM_STEPS, NTMR };
// TM_STATE's values, include/mpcekf.h's MPCEKF_TERM_*
enum { TERM_OPEN = 0, TERM_LATCHED, TERM_DEAD };
// rows of the parameters [NTMP][n]
enum { TMP_SOC_STOP = 0, TMP_I_TAPER, TMP_T_CUT, NTMP };
// REASON's bits
enum { TERM_R_SOC = 1, TERM_R_TAPER = 2, TERM_R_TEMP = 4, TERM_R_STRING = 8 };

constexpr int TERM_BLOCK = 256;

struct KTerm {
  double *uk, *uk_1;   // [n] s.uk: each cell's command, +0.0 for a latched cell; s.uk_1 likewise
  double *u;           // [n] this step's u row of the call's outputs, may be null
  const double *soc;   // [n] this step's soc row (the call's, or the context's scratch row)
  const double *Tc;    // [n] s.Tc: the temperature the step used
  const double *par;   // [NTMP][n]
  double *rec;         // [NTMR][n]
  int *cnt;            // [2][n] the taper counter: armed, run
  const int *flag_in;  // [n / series] strings with a latched cell after the previous step; null: no strings
  int *flag_out;       // [n / series] the same after this step (the other half of the pair); null likewise
  int *open;           // [1] the number of OPEN cells
  int64_t n;
  int series;          // cells per string (1 without a pack)
  int hold;
};

// the record and the counters as mpcekf_term_begin leaves them; *open = n
int launch_term_reset(double *rec, int *cnt, int *flags, int *open, int64_t n, void *stream);
// once per call on a pack context: flag[g] = 1 for every string g that holds a latched cell
// (the flags are zeroed by the caller first)
int launch_term_seed(const double *rec, int *flag, int64_t n, int series, void *stream);
// one step's rule, after the step's Hildreth (and k_cl_diag), before k_pack
int launch_term(const KTerm &q, void *stream);

}  // namespace mk
