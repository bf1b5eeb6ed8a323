// mpcekf_balance.hpp -- passive balancing of pack strings along the fused loop
// (mpcekf_balance_begin): the record's and the parameters' rows, the kernel's arguments and the
// launches of mpcekf_balance.hip.  Not a reference function: runMPC.m charges one cell; a
// balancer diverts part of a string's current around the cells that are ahead.
#pragma once

#include <cstdint>

#include "mpcekf_pack.hpp"

namespace mk {

// rows of the parameters [NBLP][n] and of the record [NBLR][n], in the order of
// include/mpcekf.h's MPCEKF_BLP_* / MPCEKF_BL_* (checked in mpcekf_host.cpp)
enum { BLP_I_BLEED = 0, BLP_DZ_ON, BLP_DZ_OFF, NBLP };
enum { BL_STEPS_ON = 0, BL_Q_BLEED, BL_SWITCHES, BL_DZ_MAX, BL_DZ_LAST, BL_STEPS, NBLR };

struct KPackBal {
  KPack p;            // k_pack's arguments: s.uk, s.uk_1, the u / ucmd / limiter rows, the pack record, n, series
  const double *soc;  // [n] this step's soc row (the call's, the summary window's or the context's own)
  const double *par;  // [NBLP][n]
  int *on;            // [n] the cells' flags
  double *rec;        // [NBLR][n]
  double *bleed;      // [n] this step's row of bleed currents, may be null
  double *zmin;       // [n / series] this step's row of the strings' smallest soc, may be null
  int compensate;     // 0 / 1
};

// the flags to 0, the record to its start (counts and sums +0.0, DZ_MAX and DZ_LAST NaN)
int launch_bal_reset(double *rec, int *on, int64_t n, void *stream);
// one step's balancing and coupling, in launch_pack's place: after k_term, before the summary
// fold and k_thermal
int launch_pack_bal(const KPackBal &q, void *stream);

}  // namespace mk
