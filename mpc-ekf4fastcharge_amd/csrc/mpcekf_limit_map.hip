// mpcekf_limit_map.hip -- the MPC limits mapped over (SOC estimate, cell temperature)
// (include/mpcekf.h, mpcekf_limit_map): for every mapped field the MPC stage of fused step t reads
// the 2-D table value at the soc row of step t - 1 and the temperature step t uses, so a
// multi-stage constant-current map, or a plating margin that widens towards the top of charge,
// runs inside the fused loop.  Not a reference function.
//
// Placement.  The estimate of step t is formed inside k_cell, after which the same kernel's MPC
// stage already reads the limits, so the map is evaluated at the estimate of step t - 1: each
// step's last launch stores the step's soc row into the record's Z_LAST row and, when another step
// of the call follows, evaluates the map there and at the temperature that step will find.
//   - without a thermal model: k_map_step, one launch of one lane per cell at the end of the step;
//   - with a model: k_thermal_map in k_thermal's place -- k_thermal statement for statement, then
//     Z_LAST and the map at the temperature it leaves -- so the map adds no launch;
//   - with thermal links: k_thermal_couple as before, then k_map_step at s.Tc as it leaves it.
// A call evaluates once before its first step (k_map) at Z_LAST and s.Tc as they stand, which
// picks up whatever init_cells, thermal_begin or a stage call stored since the last call.  The
// call's last step stores Z_LAST and evaluates nothing, so the values in force after a call are
// those its last step used.
//
// One lane per cell.  Per mapped field a cell loads up to four neighbouring table entries (the
// tables are a few thousand doubles, read-only, served from L2 / the vector cache) and stores two
// or three doubles.  The header is wave-uniform.  No LDS, no atomics, plain vector stores.
//
// Every operation of the lookup is one separately rounded fp64 operation in the order
// include/mpcekf.h spells out (no contraction, IEEE division); tests/limit_map_ref.py restates
// it in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_kernels.hpp"
#include "mpcekf_limit_map.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

__device__ __forceinline__ bool isnan_(double x) { return x != x; }

__global__ void __launch_bounds__(256) k_map_reset(double *rec, int keep, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  if (!keep) rec[(int64_t)LM_Z_LAST * n + c] = __builtin_nan("");
  rec[(int64_t)LM_NEVAL * n + c] = 0.0;
  rec[(int64_t)LM_NCLAMP_Z * n + c] = 0.0;
  rec[(int64_t)LM_NCLAMP_T * n + c] = 0.0;
}

__global__ void __launch_bounds__(256) k_map(KMap g) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.n) return;
  map_eval(g, c, g.rec[(int64_t)LM_Z_LAST * g.n + c], g.Tc[c]);
}

__global__ void __launch_bounds__(256) k_map_step(KMap g) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= g.n) return;
  const double z = g.soc[c];
  g.rec[(int64_t)LM_Z_LAST * g.n + c] = z;
  if (g.eval) map_eval(g, c, z, g.Tc[c]);
}

// k_thermal (mpcekf_thermal.hip) statement for statement, then the map at the temperature the
// next step will find.  k_thermal itself stays as it is for a context without a map.
__global__ void __launch_bounds__(256) k_thermal_map(KTherm q, KMap g) {
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
  const double zs = g.soc[c];
  g.rec[(int64_t)LM_Z_LAST * n + c] = zs;
  if (g.eval) map_eval(g, c, zs, Tnext);
}

inline dim3 grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

int launch_map_reset(double *rec, int keep, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_map_reset, grid(n), dim3(256), 0, (hipStream_t)stream, rec, keep, n);
  return (int)hipGetLastError();
}

int launch_map(const KMap &g, void *stream) {
  if (g.n <= 0) return 0;
  hipLaunchKernelGGL(k_map, grid(g.n), dim3(256), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_map_step(const KMap &g, void *stream) {
  if (g.n <= 0) return 0;
  hipLaunchKernelGGL(k_map_step, grid(g.n), dim3(256), 0, (hipStream_t)stream, g);
  return (int)hipGetLastError();
}

int launch_thermal_map(const KTherm &q, const KMap &g, void *stream) {
  if (q.n <= 0) return 0;
  hipLaunchKernelGGL(k_thermal_map, grid(q.n), dim3(256), 0, (hipStream_t)stream, q, g);
  return (int)hipGetLastError();
}

}  // namespace mk
