// mpcekf_dexp.hpp -- the defined exp, one definition for every unit that evaluates it: the v3
// Arrhenius factor of the electrode lookups (mpcekf_kernels.hip) and the side-reaction currents
// of mpcekf_aging.hip.
#pragma once

#include <hip/hip_runtime.h>

namespace mk {

namespace dm {
constexpr double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
}  // namespace dm

// Defined exp of the v3 Arrhenius factor (oracle/mpcekf_oracle.c orc_exp, rom.py dexp):
// x = k ln2 + r, k = floor(x / ln2 + 1/2), fdlibm's rational form for exp(r); only
// +, -, *, /, floor and ldexp, exact or correctly rounded on both sides.
// The special cases by selects (the in-range arithmetic unchanged), so that a lookup is one
// basic block and neighbouring lookups' L2 loads can overlap (profiles/r05h_ab_branchfree.txt)
__device__ __forceinline__ double dexp(double x0) {
  const bool nan = x0 != x0, big = x0 > 709.782712893384, small = x0 < -745.1332191019412;
  const double x = (nan || big || small) ? 0.0 : x0;
  const double k = floor(x * 1.44269504088896338700e+00 + 0.5);
  const double hi = x - k * dm::LN2_HI;
  const double lo = k * dm::LN2_LO;
  const double r = hi - lo;
  const double t = r * r;
  const double c = r - t * (1.66666666666666019037e-01 +
                            t * (-2.77777777770155933842e-03 +
                                 t * (6.61375632143793436117e-05 +
                                      t * (-1.65339022054652515390e-06 + t * 4.13813679705723846039e-08))));
  const double y = 1.0 - ((lo - (r * c) / (2.0 - c)) - hi);
  const double v = ldexp(y, (int)k);
  return nan ? x0 : big ? __builtin_inf() : small ? 0.0 : v;
}

}  // namespace mk
