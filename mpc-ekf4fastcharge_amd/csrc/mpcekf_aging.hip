// mpcekf_aging.hip -- side-reaction losses per cell along the fused loop (include/mpcekf.h,
// mpcekf_aging_begin): after fused step t every reaction's Tafel current at the step's
// side-reaction overpotential and temperature is added to the cell's record, for the EKF's
// estimate (phise_store), the plant's own negPhise0, or both.  Not a reference function.
//
// k_aging is launched once per fused step, one lane per cell, after the kernel that wrote the
// step's phise row and before k_thermal advances s.Tc.  Both sources share the launch; the source
// and reaction loops run over kernel arguments, so they are wave-uniform.  Parameters and record
// are slot-major [..][n]: every access of a wave is one run of consecutive doubles.  Per cell,
// source and reaction it loads 5 parameters and 4 record rows and stores the 4 rows back (and a
// rate row when asked for); per cell and source the phi value and the two step counters.  No
// LDS, no atomics, plain vector stores.  The record is read-modify-written by the cell's own
// lane in step order, which is what makes Q_SUM the sequential sum the header defines.
//
// The step index of J_MAX_STEP is the record's STEPS + NSKIP + 1: read from the record, never
// passed as an argument, so a captured graph replays correctly on a later call.
//
// Every operation below is one separately rounded fp64 operation in the order include/mpcekf.h
// spells out (no contraction, IEEE division, the project's dexp); tests/aging_ref.py restates
// it in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_aging.hpp"

#pragma clang fp contract(off)

#include "mpcekf_dexp.hpp"

namespace mk {
namespace {

__device__ __forceinline__ bool isnan_(double x) { return x != x; }

__global__ void __launch_bounds__(256) k_aging_reset(double *rec, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double NaN = __builtin_nan("");
  for (int s = 0; s < AG_NSRC; ++s) {
    for (int r = 0; r < AG_MAXR; ++r) {
      rec[(int64_t)ag_row(s, r, AGR_Q_SUM) * n + c] = 0.0;
      rec[(int64_t)ag_row(s, r, AGR_J_MAX) * n + c] = NaN;
      rec[(int64_t)ag_row(s, r, AGR_J_MAX_STEP) * n + c] = 0.0;
      rec[(int64_t)ag_row(s, r, AGR_N_ON) * n + c] = 0.0;
    }
    rec[(int64_t)ag_row(s, 0, AGR_STEPS) * n + c] = 0.0;
    rec[(int64_t)ag_row(s, 0, AGR_NSKIP) * n + c] = 0.0;
  }
}

__global__ void __launch_bounds__(256) k_aging(KAging q) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = q.n;
  if (c >= n) return;
  const double NaN = __builtin_nan("");
  const double T = q.Tc[c];
  const double TK = T + 273.15;
  const double RT = q.R * TK;
  const double dinv = 1.0 / q.Tref - 1.0 / TK;
  int out = 0;  // the rate block's row: enabled sources in id order, reactions inside
  for (int s = 0; s < AG_NSRC; ++s) {
    if (!q.phi[s]) continue;
    const double phi = q.phi[s][c];
    const bool skip = isnan_(phi);
    double *S = q.rec + (int64_t)ag_row(s, 0, AGR_STEPS) * n + c;
    double steps = S[0], nskip = S[n];
    const double tt = (steps + nskip) + 1.0;
    for (int r = 0; r < q.nreact; ++r) {
      const double *P = q.par + (int64_t)r * NAGP * n + c;
      const double i0 = P[AG_I0 * n], U = P[AG_U * n], alpha = P[AG_ALPHA * n], Ea = P[AG_EA * n];
      const double gate = P[AG_GATE * n];
      double *R = q.rec + (int64_t)ag_row(s, r, AGR_Q_SUM) * n + c;
      double qsum = R[AGR_Q_SUM * n], jmax = R[AGR_J_MAX * n], jstep = R[AGR_J_MAX_STEP * n], non = R[AGR_N_ON * n];
      const double eta = phi - U;
      const double g = (alpha * q.F) / RT;
      const double ar = dexp((Ea / q.R) * dinv);
      const double j = (i0 * ar) * dexp(-(g * eta));
      const bool take = eta < gate && __builtin_isfinite(j);  // a NaN eta compares false
      if (take) {
        qsum = qsum + j;
        non = non + 1.0;
        if (isnan_(jmax) || j > jmax) {
          jmax = j;
          jstep = tt;
        }
      }
      R[AGR_Q_SUM * n] = qsum;
      R[AGR_J_MAX * n] = jmax;
      R[AGR_J_MAX_STEP * n] = jstep;
      R[AGR_N_ON * n] = non;
      if (q.rate) q.rate[(int64_t)out * n + c] = skip ? NaN : take ? j : 0.0;
      ++out;
    }
    if (skip) {
      nskip = nskip + 1.0;
    } else {
      steps = steps + 1.0;
    }
    S[0] = steps;
    S[n] = nskip;
  }
}

}  // namespace

int launch_aging_reset(double *rec, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_aging_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec, n);
  return (int)hipGetLastError();
}

int launch_aging(const KAging &q, void *stream) {
  if (q.n <= 0) return 0;
  hipLaunchKernelGGL(k_aging, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}

}  // namespace mk
