// mpcekf_thermal.hip -- the per-cell lumped thermal model of the fused loop (include/mpcekf.h,
// mpcekf_thermal_begin): after fused step t the cell temperature s.Tc advances by the heat the
// step generated, q = i (U(z) - v), less the loss to the ambient, so the next step's OB_step,
// iterEKF and EKFmatsHandler (runMPC.m:85-92's TC) read a temperature that follows from the
// charge itself.  Not a reference function.
//
// k_thermal is launched last in each fused step, one lane per cell.  Per cell it loads 15
// scalars (T, the applied current, s.uk, s.vk, SOCnAvg, the three parameters, the six stored
// record rows: 14 doubles, and the status word: 116 B) and two neighbouring table entries, and
// stores 7 to 10 doubles (the applied current for the next step and the six record rows
// always; T when it advances; the temp and heat rows when asked for: 56-80 B).  No LDS, no
// atomics, plain stores.  The OCV table (at most a few hundred doubles, read-only) stays in
// global memory and is served from L2 / the vector cache.
//
// The applied current: the step's kernels overwrite s.uk with the next command, so the host
// copies s.uk into q.iapp once, before a call's first step; from then on k_thermal itself
// stores the s.uk it finds after step t into q.iapp, which is the current step t + 1 applies
// (nothing writes s.uk between two steps of a call).
//
// The step index of T_MAX_STEP is the record's STEPS + NHELD + 1: read from the record, never
// passed as an argument, so a captured graph replays correctly on a later call.
//
// Every operation below is one separately rounded fp64 operation in the order include/mpcekf.h
// spells out (no contraction, IEEE division); tests/test_gpu_thermal.py restates it in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_kernels.hpp"
#include "mpcekf_thermal.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

__device__ __forceinline__ bool isnan_(double x) { return x != x; }

__global__ void __launch_bounds__(256) k_thermal_reset(double *rec, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double NaN = __builtin_nan("");
  rec[(int64_t)THR_T_MAX * n + c] = NaN;
  rec[(int64_t)THR_T_MAX_STEP * n + c] = 0.0;
  rec[(int64_t)THR_T_MIN * n + c] = NaN;
  rec[(int64_t)THR_HEAT_SUM * n + c] = 0.0;
  rec[(int64_t)THR_STEPS * n + c] = 0.0;
  rec[(int64_t)THR_NHELD * n + c] = 0.0;
}

__global__ void __launch_bounds__(256) k_thermal(KTherm q) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = q.n;
  if (c >= n) return;
  const double T = q.Tc[c];
  const double i = q.iapp[c];
  // voltage_store(t): a cell in error has NaN outputs from its failing step on, whatever the
  // plant left in s.vk before the EKF refused the step
  const double v = (q.status[c] & ST_ERROR) ? __builtin_nan("") : q.vk[c];
  const double Cth = q.par[(int64_t)TH_CTH * n + c], Rth = q.par[(int64_t)TH_RTH * n + c];
  const double Tamb = q.par[(int64_t)TH_TAMB * n + c];
  double *R = q.rec + c;
  double tmax = R[THR_T_MAX * n], tmax_t = R[THR_T_MAX_STEP * n], tmin = R[THR_T_MIN * n];
  double hsum = R[THR_HEAT_SUM * n], steps = R[THR_STEPS * n], nheld = R[THR_NHELD * n];
  q.iapp[c] = q.uk[c];  // the current the next step applies

  const double z = (q.SOCn[c] - q.th0n) / (q.th100n - q.th0n);  // OB_step.m:228
  double zc = z > 0.0 ? z : 0.0;                                // NaN -> 0
  zc = zc < 1.0 ? zc : 1.0;
  const double s = zc * (double)(q.nocv - 1);
  int j = (int)s;
  if (j > q.nocv - 2) j = q.nocv - 2;
  const double f = s - (double)j;
  const double u0 = q.ocv[j], u1 = q.ocv[j + 1];
  const double U = u0 + f * (u1 - u0);
  const double heat = i * (U - v);
  const double loss = (T - Tamb) / Rth;
  const double Tn = T + ((heat - loss) * q.Ts) / Cth;

  const double t = (steps + nheld) + 1.0;
  if (isnan_(tmax) || T > tmax) {
    tmax = T;
    tmax_t = t;
  }
  if (isnan_(tmin) || T < tmin) tmin = T;
  if (__builtin_isfinite(heat)) hsum = hsum + heat;
  if (__builtin_isfinite(Tn) && Tn <= 100.0) {  // check_tc's rule
    q.Tc[c] = Tn;
    steps = steps + 1.0;
  } else {
    nheld = nheld + 1.0;
  }
  R[THR_T_MAX * n] = tmax;
  R[THR_T_MAX_STEP * n] = tmax_t;
  R[THR_T_MIN * n] = tmin;
  R[THR_HEAT_SUM * n] = hsum;
  R[THR_STEPS * n] = steps;
  R[THR_NHELD * n] = nheld;
  if (q.temp) q.temp[c] = T;
  if (q.heat) q.heat[c] = heat;
}

}  // namespace

int launch_thermal_reset(double *rec, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_thermal_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec, n);
  return (int)hipGetLastError();
}

int launch_thermal(const KTherm &q, void *stream) {
  if (q.n <= 0) return 0;
  hipLaunchKernelGGL(k_thermal, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}

}  // namespace mk
