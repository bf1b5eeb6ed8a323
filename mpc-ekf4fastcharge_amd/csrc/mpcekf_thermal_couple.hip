// mpcekf_thermal_couple.hip -- heat conduction between neighbouring cells of a pack string
// (include/mpcekf.h, mpcekf_thermal_couple): the thermal model's step of mpcekf_thermal.hip with
// one more heat flow per link, qn = (Tl - T) / r_link[c-1] + (Tr - T) / r_link[c], added to the
// cell's own q - loss before the temperature advances.  Not a reference function.
//
// k_thermal_couple takes k_thermal's place as the step's last launch on a coupled context, and
// k_thermal_couple_sched takes k_thermal_sched's place; one lane per cell.  Over k_thermal a lane
// loads up to two links and two neighbour temperatures (coalesced: the lines its own loads and
// its wave's hit) and the three record rows, and stores one more temperature and the record.
// No LDS, no atomics, plain vector loads and stores.
//
// The hazard and the snapshot.  s.Tc is advanced in place, and this is the one kernel of the
// fused step in which a lane reads what a lane of another wave or block writes in the same
// launch: read from s.Tc, a neighbour's temperature would be T or Tn by block scheduling.  So no
// lane reads a neighbour from s.Tc.  The context keeps a ping-pong pair snap[2][n]:
//   - k_couple_seed, once at the start of every fused call, copies s.Tc to snap[0] (whatever
//     init_cells, thermal_begin's t0 or a stage call's temperature argument stored since the last
//     call is picked up here);
//   - the kernel of the call's k-th step (from 0) reads its neighbours from snap[k & 1], which no
//     lane of this launch writes, and stores the temperature it leaves, advanced or held, to
//     snap[(k + 1) & 1], which no lane of this launch reads.
// Within a launch every address is written by one lane at most and no lane reads an address
// another lane writes; launches of one stream run in order.  So the result does not depend on
// how blocks are scheduled.  The parity is call-relative: a captured graph names the same
// buffers on every replay.
//
// Every operation is one separately rounded fp64 operation in the order include/mpcekf.h spells
// out (no contraction, IEEE division); tests/couple_ref.py restates it in numpy.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "mpcekf_kernels.hpp"
#include "mpcekf_thermal_couple.hpp"

#pragma clang fp contract(off)

namespace mk {
namespace {

__device__ __forceinline__ bool isnan_(double x) { return x != x; }

// k_thermal's statements (mpcekf_thermal.hip), written once for the kernels of this file, with
// the neighbours' heat flow qn over nl links in the advance.  T is s.Tc[c], already loaded.
// Returns the temperature the step leaves (Tn, or T when held); *t_out is the model's step index.
__device__ __forceinline__ double thermal_body(const KTherm &q, int64_t c, double T, double qn, int nl, double *t_out) {
  const int64_t n = q.n;
  const double i = q.iapp[c];
  // voltage_store(t): a cell in error has NaN outputs from its failing step on
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
  // no link: the uncoupled line, bit for bit (x + 0.0 is x for every x but -0.0)
  const double Tn = nl == 0 ? T + ((heat - loss) * q.Ts) / Cth : T + (((heat - loss) + qn) * q.Ts) / Cth;

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
  *t_out = t;
  return Tnext;
}

// cell c's step with conduction; returns the temperature it leaves.  The neighbours c - 1 and
// c + 1 are read only inside c's string, so both indices are inside [0, n): series divides n.
__device__ __forceinline__ double couple_step(const KTherm &q, const KCouple &h, int64_t c) {
  const int64_t n = q.n;
  const double T = q.Tc[c];
  const int64_t p = c % h.series, S = h.series;
  double qn = 0.0;
  int nl = 0;
  double dmax = __builtin_nan("");  // this step's largest |dl|, |dr|: the left link first
  if (p > 0) {
    const double r = h.rlink[c - 1];
    if (__builtin_isfinite(r)) {
      const double dl = h.snap_in[c - 1] - T;
      qn = qn + dl / r;
      nl += 1;
      dmax = __builtin_fabs(dl);
    }
  }
  if (p < S - 1) {
    const double r = h.rlink[c];
    if (__builtin_isfinite(r)) {
      const double dr = h.snap_in[c + 1] - T;
      qn = qn + dr / r;
      nl += 1;
      const double a = __builtin_fabs(dr);
      if (isnan_(dmax) || a > dmax) dmax = a;
    }
  }
  double t;
  const double Tnext = thermal_body(q, c, T, qn, nl, &t);
  h.snap_out[c] = Tnext;
  if (nl > 0) {
    double *R = h.rec + c;
    if (__builtin_isfinite(qn)) R[TCR_NB_SUM * n] = R[TCR_NB_SUM * n] + qn;
    const double old = R[TCR_DT_MAX * n];
    if (isnan_(old) || dmax > old) {
      R[TCR_DT_MAX * n] = dmax;
      R[TCR_DT_MAX_STEP * n] = t;
    }
  }
  if (h.cond) h.cond[c] = qn;
  return Tnext;
}

__global__ void __launch_bounds__(256) k_couple_reset(double *rec, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  rec[(int64_t)TCR_NB_SUM * n + c] = 0.0;
  rec[(int64_t)TCR_DT_MAX * n + c] = __builtin_nan("");
  rec[(int64_t)TCR_DT_MAX_STEP * n + c] = 0.0;
}

__global__ void __launch_bounds__(256) k_couple_seed(const double *Tc, double *snap, int64_t n) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  snap[c] = Tc[c];
}

__global__ void __launch_bounds__(256) k_thermal_couple(KTherm q, KCouple h) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= q.n) return;
  (void)couple_step(q, h, c);
}

__global__ void __launch_bounds__(256) k_thermal_couple_sched(KTherm q, KCouple h, KSched g) {
  const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= q.n) return;
  sched_eval(g, c, couple_step(q, h, c));
}

inline dim3 grid(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }

}  // namespace

int launch_couple_reset(double *rec, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_couple_reset, grid(n), dim3(256), 0, (hipStream_t)stream, rec, n);
  return (int)hipGetLastError();
}

int launch_couple_seed(const double *Tc, double *snap, int64_t n, void *stream) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_couple_seed, grid(n), dim3(256), 0, (hipStream_t)stream, Tc, snap, n);
  return (int)hipGetLastError();
}

int launch_thermal_couple(const KTherm &q, const KCouple &h, void *stream) {
  if (q.n <= 0) return 0;
  hipLaunchKernelGGL(k_thermal_couple, grid(q.n), dim3(256), 0, (hipStream_t)stream, q, h);
  return (int)hipGetLastError();
}

int launch_thermal_couple_sched(const KTherm &q, const KCouple &h, const KSched &g, void *stream) {
  if (q.n <= 0) return 0;
  hipLaunchKernelGGL(k_thermal_couple_sched, grid(q.n), dim3(256), 0, (hipStream_t)stream, q, h, g);
  return (int)hipGetLastError();
}

}  // namespace mk
