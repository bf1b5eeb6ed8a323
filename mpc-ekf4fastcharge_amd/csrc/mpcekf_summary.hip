// mpcekf_summary.hip -- the per-cell charge summary of mpcekf_step_summary (include/mpcekf.h,
// MPCEKF_SUM_*): a streaming reduction of the fused step's per-step outputs (runMPC.m:94-111's
// u_store, voltage_store, SOC_store, phise_store and mpcData.cost.nexec, plus one slot of
// OB_step's obs) over the steps of a charge, kept on the device.  Not a reference function.
//
// During mpcekf_step_summary the fused step writes those rows into a SUM_WIN-row ring instead
// of [nsteps][ncells] trajectories; k_summary folds a window of the ring into the record once
// per SUM_WIN steps and at the end of a call.  One lane per cell: the lane loads its
// accumulators, walks the window's rows in step order (row[k n + c]: consecutive lanes on
// consecutive cells, the loads of PF rows issued before the first is used) and stores the
// accumulators once.  No LDS, no atomics, plain stores.
//
// The step index t of a row is the record's SEEN + 1, + 2, ...: it is read from the record and
// never passed as an argument, so a captured graph replays correctly on a later call.
// Every rule that decides a bit (strict comparisons, the first occurrence wins, the sum in
// step order) is restated in tests/summary_ref.py.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_summary.hpp"

namespace mk {
namespace {

constexpr int PF = 4;  // rows in flight per lane (6 loads each)

__device__ __forceinline__ bool isnan_(double x) { return x != x; }

// a smaller / larger value replaces the extremum only on a strict comparison (the first
// occurrence wins; -0 and +0 do not displace each other); NaN = no value yet
__device__ __forceinline__ void take_min(double x, double t, double &m, double &mt) {
  if (isnan_(m) || x < m) {
    m = x;
    mt = t;
  }
}
__device__ __forceinline__ void take_max(double x, double t, double &m, double &mt) {
  if (isnan_(m) || x > m) {
    m = x;
    mt = t;
  }
}

__global__ void __launch_bounds__(256) k_summary_reset(double *rec, double *reach, int no_reach, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double NaN = __builtin_nan("");
#pragma unroll
  for (int f = 0; f < NSUM; ++f) {
    const bool count = f == SUM_SEEN || f == SUM_STEPS || f == SUM_ERR_STEP || f == SUM_T_REACH ||
                       f == SUM_U_MIN_STEP || f == SUM_V_MAX_STEP || f == SUM_PHISE_MIN_STEP || f == SUM_U_SUM ||
                       f == SUM_NEXEC_SUM || f == SUM_NSAT || f == SUM_OBS_MIN_STEP || f == SUM_OBS_MAX_STEP;
    rec[(int64_t)f * n + c] = count ? 0.0 : NaN;
  }
  if (no_reach) reach[c] = NaN;
}

__global__ void __launch_bounds__(256) k_summary(KSum q) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t n = q.n;
  if (c >= n) return;
  double *R = q.rec + c;
  double seen = R[SUM_SEEN * n], steps = R[SUM_STEPS * n], err = R[SUM_ERR_STEP * n], treach = R[SUM_T_REACH * n];
  double umin = R[SUM_U_MIN * n], umin_t = R[SUM_U_MIN_STEP * n], umax = R[SUM_U_MAX * n];
  double vmax = R[SUM_V_MAX * n], vmax_t = R[SUM_V_MAX_STEP * n], vmin = R[SUM_V_MIN * n];
  double pmin = R[SUM_PHISE_MIN * n], pmin_t = R[SUM_PHISE_MIN_STEP * n];
  double ulast = R[SUM_U_LAST * n], vlast = R[SUM_V_LAST * n], slast = R[SUM_SOC_LAST * n];
  double plast = R[SUM_PHISE_LAST * n], usum = R[SUM_U_SUM * n];
  double nesum = R[SUM_NEXEC_SUM * n], nemax = R[SUM_NEXEC_MAX * n], nsat = R[SUM_NSAT * n];
  double omin = R[SUM_OBS_MIN * n], omin_t = R[SUM_OBS_MIN_STEP * n];
  double omax = R[SUM_OBS_MAX * n], omax_t = R[SUM_OBS_MAX_STEP * n];
  const double reach = q.reach[c];
  const bool has_obs = q.obs != nullptr;
  const int nrows = q.nrows;
  double unused = 0.0;
  for (int k0 = 0; k0 < nrows; k0 += PF) {
    double u[PF], v[PF], s[PF], p[PF], o[PF];
    int ne[PF];
#pragma unroll
    for (int j = 0; j < PF; ++j) {  // the tail repeats the last row's loads; they are not used
      const int64_t i = (int64_t)(k0 + j < nrows ? k0 + j : nrows - 1) * n + c;
      u[j] = q.u[i];
      v[j] = q.v[i];
      s[j] = q.soc[i];
      p[j] = q.phise[i];
      ne[j] = q.nexec[i];
      o[j] = has_obs ? q.obs[i] : 0.0;
    }
#pragma unroll
    for (int j = 0; j < PF; ++j) {
      if (k0 + j >= nrows) break;
      seen = seen + 1.0;
      const double t = seen;
      // a counted step: none of its u, v, soc, phise is NaN (a cell in error has NaN outputs)
      if (!(isnan_(u[j]) || isnan_(v[j]) || isnan_(s[j]) || isnan_(p[j]))) {
        steps = steps + 1.0;
        if (treach == 0.0 && s[j] >= reach) treach = t;
        take_min(u[j], t, umin, umin_t);
        take_max(u[j], t, umax, unused);
        take_max(v[j], t, vmax, vmax_t);
        take_min(v[j], t, vmin, unused);
        take_min(p[j], t, pmin, pmin_t);
        ulast = u[j];
        vlast = v[j];
        slast = s[j];
        plast = p[j];
        usum = usum + u[j];  // in step order
        const double x = (double)ne[j];
        nesum = nesum + x;
        take_max(x, t, nemax, unused);
        if (ne[j] >= q.max_hild) nsat = nsat + 1.0;
      } else if (err == 0.0) {
        err = t;
      }
      if (has_obs && !isnan_(o[j])) {  // the plant's slot: its own NaN steps are skipped
        take_min(o[j], t, omin, omin_t);
        take_max(o[j], t, omax, omax_t);
      }
    }
  }
  R[SUM_SEEN * n] = seen;
  R[SUM_STEPS * n] = steps;
  R[SUM_ERR_STEP * n] = err;
  R[SUM_T_REACH * n] = treach;
  R[SUM_U_MIN * n] = umin;
  R[SUM_U_MIN_STEP * n] = umin_t;
  R[SUM_U_MAX * n] = umax;
  R[SUM_V_MAX * n] = vmax;
  R[SUM_V_MAX_STEP * n] = vmax_t;
  R[SUM_V_MIN * n] = vmin;
  R[SUM_PHISE_MIN * n] = pmin;
  R[SUM_PHISE_MIN_STEP * n] = pmin_t;
  R[SUM_U_LAST * n] = ulast;
  R[SUM_V_LAST * n] = vlast;
  R[SUM_SOC_LAST * n] = slast;
  R[SUM_PHISE_LAST * n] = plast;
  R[SUM_U_SUM * n] = usum;
  R[SUM_NEXEC_SUM * n] = nesum;
  R[SUM_NEXEC_MAX * n] = nemax;
  R[SUM_NSAT * n] = nsat;
  if (has_obs) {
    R[SUM_OBS_MIN * n] = omin;
    R[SUM_OBS_MIN_STEP * n] = omin_t;
    R[SUM_OBS_MAX * n] = omax;
    R[SUM_OBS_MAX_STEP * n] = omax_t;
  }
}

}  // namespace

int launch_summary_reset(double *rec, double *reach, bool no_reach, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_summary_reset, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, rec, reach,
                     no_reach ? 1 : 0, n);
  return (int)hipGetLastError();
}

int launch_summary(const KSum &q, void *stream) {
  if (q.n <= 0 || q.nrows <= 0) return 0;
  hipLaunchKernelGGL(k_summary, dim3((unsigned)((q.n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, q);
  return (int)hipGetLastError();
}

}  // namespace mk
