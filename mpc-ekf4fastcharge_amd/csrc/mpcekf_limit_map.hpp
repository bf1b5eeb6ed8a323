// mpcekf_limit_map.hpp -- the MPC limits mapped over (SOC estimate, cell temperature)
// (mpcekf_limit_map): the map's device header, the record's rows, the kernels' arguments and the
// launches of mpcekf_limit_map.hip.  Not a reference function: runMPC.m:30-44 sets its limits once.
#pragma once

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#endif

#include <cstdint>

#include "mpcekf_thermal.hpp"

namespace mk {

enum { MAP_MAXF = 6 };  // the fields a map can hold: CRATE, U_MAX, DU_MIN, DU_MAX, V_MAX, PHISE_MIN

// rows of the record [NLMR][n], in the order of include/mpcekf.h's MPCEKF_LM_* (checked in
// mpcekf_host.cpp)
enum { LM_Z_LAST = 0, LM_NEVAL, LM_NCLAMP_Z, LM_NCLAMP_T, NLMR };

// The map as the kernels read it, in device memory: every quantity a replaced map may change
// lives here or in the buffers below, none in a kernel argument, so a captured graph replays the
// map in force.
struct MapHdr {
  double z_lo, z_hi;      // the SOC grid's ends (fractions)
  double T_lo, T_hi;      // the temperature grid's ends, degC (unused with nt == 1)
  double Q;               // rom.Q: the CRATE slot is u_min = -Q * val (fill_kcfg's expression)
  int nz, nt, interp_z;   // interp_z 1: hold (the left node's value)
  int nf, nsets, pad;
  int slot[MAP_MAXF];     // field i's row LK_* of the limits record
  int crate[MAP_MAXF];    // 1: field i is CRATE
};

struct KMap {
  const MapHdr *hdr;
  const double *tab;  // [nsets][nf][nt][nz]
  const int *set;     // [n] each cell's table set, 0..nsets-1 (checked by the host)
  const double *Tc;   // [n] s.Tc (read only with nt >= 2)
  const double *soc;  // [n] this step's soc row (k_map_step, k_thermal_map); null for k_map
  double *lim;        // [NLIMK][n] mpcekf_set_limits' record: row slot[i] written
  double *val;        // [MAP_MAXF][n] the values in force, mpcekf_config units: row i written
  double *rec;        // [NLMR][n]
  double *out;        // [nf][n] the evaluated values' block of the call's lim rows, may be null
  int64_t n;
  int eval;           // k_map_step, k_thermal_map: 0 on a call's last step, which evaluates nothing
  int count;          // 1: the evaluation belongs to a fused step (NEVAL, NCLAMP_* advance)
};

// the record's counts reset; Z_LAST to NaN, or (keep) left as it is
int launch_map_reset(double *rec, int keep, int64_t n, void *stream);
// the map at every cell's Z_LAST and temperature as they stand (before a call's first step, and
// when a map is set)
int launch_map(const KMap &g, void *stream);
// the last launch of a step on a context without a thermal model, or after k_thermal_couple:
// Z_LAST from the step's soc row, then (g.eval) the map there and at s.Tc as it stands
int launch_map_step(const KMap &g, void *stream);
// k_thermal's step of the model, Z_LAST from the step's soc row, then (g.eval) the map there and
// at the temperature the model leaves: a step's last kernel on a thermal context
int launch_thermal_map(const KTherm &q, const KMap &g, void *stream);

#ifdef __HIPCC__
// The lookup, written once for every kernel that evaluates the map.  Every operation is one
// separately rounded fp64 operation in the order include/mpcekf.h spells out: the including file
// sets `#pragma clang fp contract(off)` before its kernels.
#pragma clang fp contract(off)
// one axis: the column j and the weight f of argument a on a uniform grid of m >= 2 nodes;
// returns 1 when the argument fell outside the grid or was NaN
static __device__ __forceinline__ int map_axis(double a, double lo, double hi, int m, int *j_out, double *f_out) {
  const double x = (a - lo) / (hi - lo);
  double xc = x > 0.0 ? x : 0.0;  // NaN -> 0
  xc = xc < 1.0 ? xc : 1.0;
  const double s = xc * (double)(m - 1);
  int j = (int)s;
  if (j > m - 2) j = m - 2;
  *j_out = j;
  *f_out = s - (double)j;
  return !(x >= 0.0 && x <= 1.0);
}

// cell c's mapped fields at SOC estimate z and temperature T
static __device__ __forceinline__ void map_eval(const KMap &g, int64_t c, double z, double T) {
  const MapHdr *h = g.hdr;
  const int64_t n = g.n;
  const int nf = h->nf, nz = h->nz, nt = h->nt;
  const double Q = h->Q;
  int jz = 0, jt = 0, cz = 0, ct = 0;
  double fz = 0.0, ft = 0.0;
  if (nz > 1) {
    cz = map_axis(z, h->z_lo, h->z_hi, nz, &jz, &fz);
    if (h->interp_z) fz = 0.0;
  } else {  // no SOC axis: the argument is still judged against the grid's ends
    const double x = (z - h->z_lo) / (h->z_hi - h->z_lo);
    cz = !(x >= 0.0 && x <= 1.0);
  }
  if (nt > 1) ct = map_axis(T, h->T_lo, h->T_hi, nt, &jt, &ft);
  const int64_t plane = (int64_t)nt * nz;
  const double *tab = g.tab + (int64_t)g.set[c] * nf * plane + (int64_t)jt * nz + jz;
  for (int i = 0; i < MAP_MAXF; ++i) {
    if (i >= nf) break;
    const double *t = tab + (int64_t)i * plane;
    double a = t[0];
    if (nz > 1) a = a + fz * (t[1] - a);
    double val = a;
    if (nt > 1) {
      double b = t[nz];
      if (nz > 1) b = b + fz * (t[nz + 1] - b);
      val = a + ft * (b - a);
    }
    g.lim[(int64_t)h->slot[i] * n + c] = h->crate[i] ? -Q * val : val;  // initMPC.m:66-67
    g.val[(int64_t)i * n + c] = val;
    if (g.out) g.out[(int64_t)i * n + c] = val;
  }
  if (g.count) {
    double *R = g.rec + c;
    R[(int64_t)LM_NEVAL * n] = R[(int64_t)LM_NEVAL * n] + 1.0;
    if (cz) R[(int64_t)LM_NCLAMP_Z * n] = R[(int64_t)LM_NCLAMP_Z * n] + 1.0;
    if (ct) R[(int64_t)LM_NCLAMP_T * n] = R[(int64_t)LM_NCLAMP_T * n] + 1.0;
  }
}
#endif  // __HIPCC__

}  // namespace mk
