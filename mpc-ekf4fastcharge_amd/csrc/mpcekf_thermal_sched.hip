// mpcekf_thermal_sched.hip -- the MPC limits scheduled over the cell temperature
// (include/mpcekf.h, mpcekf_thermal_schedule): for every scheduled field the MPC stage of fused
// step t reads the table value at the temperature step t uses, so the controller's limits follow
// the temperature the thermal model computes.  Not a reference function.
//
// Placement.  The temperature step t uses is s.Tc as the step finds it: what k_thermal left at
// the end of step t - 1, or, for a call's first step, whatever init_cells, thermal_begin or a
// stage call's temperature argument last stored.  So a call evaluates the schedule once before
// its first step (k_sched), and every step that another step of the call follows ends with
// k_thermal_sched in k_thermal's place: the model's step and then the schedule at the
// temperature it leaves, one launch instead of two.  The call's last step ends with k_thermal
// itself, so the values in force after a call are those its last step used.
//
// One lane per cell.  Per scheduled field a cell loads two neighbouring table entries (the
// tables are a few hundred doubles, read-only, served from L2 / the vector cache) and stores
// two doubles: the kernels' slot of the limits record and the value in force.  The header is
// wave-uniform.  No LDS, no atomics, plain stores.
//
// Every operation of the lookup is one separately rounded fp64 operation in the order
// include/mpcekf.h spells out (no contraction, IEEE division);
// tests/test_gpu_thermal_schedule.py restates it in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_kernels.hpp"
#include "mpcekf_thermal_sched.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

__device__ __forceinline__ bool isnan_(double x) { return x != x; }

__global__ void __launch_bounds__(256) k_sched(KSched g) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.n) return;
  sched_eval(g, c, g.Tc[c]);
}

// k_thermal (mpcekf_thermal.hip) statement for statement, then the schedule at the temperature
// the next step will find.  k_thermal itself stays as it is for a context without a schedule.
__global__ void __launch_bounds__(256) k_thermal_sched(KTherm q, KSched g) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = q.n;
  if (c >= n) return;
  const double T = q.Tc[c];
  const double i = q.iapp[c];
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
  double Tnext = T;  // held
  if (__builtin_isfinite(Tn) && Tn <= 100.0) {  // check_tc's rule
    q.Tc[c] = Tn;
    Tnext = Tn;
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
  sched_eval(g, c, Tnext);
}

}  // namespace

int launch_sched(const KSched &g, void *stream) {
  if (g.n <= 0) return 0;
  hipLaunchKernelGGL(k_sched, dim3((unsigned)((g.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_thermal_sched(const KTherm &q, const KSched &g, void *stream) {
  if (q.n <= 0) return 0;
  hipLaunchKernelGGL(k_thermal_sched, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q, g);
  return (int)hipGetLastError();
}

}  // namespace mk
